"""CPU: the episode-batch entry points refuse bad arguments without a GPU, and ``BatchedMPPI`` refuses what it does not run
before it creates an engine."""
import numpy as np
import pytest

import batched_cases as bc
from batched_cases import no_engine  # noqa: F401
from mjmpc_amd import _lib
from mjmpc_amd.models.half_cheetah import half_cheetah_raw


def test_batch_entry_points_reject_bad_arguments():
    """Null pointers, bad episode counts and sizes: a non-zero code and a message, nothing launched."""
    lib = _lib.load()
    fake = 64        # (never dereferenced: each call below fails its argument checks first)
    bad = [
        lambda: lib.mjmpc_tree_rollout_fused_batch(None, _lib.F64, 64, 8, fake, fake, None, None, fake, fake, None, None),
        lambda: lib.mjmpc_tree_step_shard_states(None, _lib.F64, fake, fake, None, None),
        lambda: lib.mjmpc_tree_get_shard_states(None, None, None, None),
        lambda: lib.mjmpc_sample_noise_batch(_lib.F64, 4, None, 8, 4, 2, fake, fake, 0, None, None),
        lambda: lib.mjmpc_sample_noise_batch(_lib.F64, 4, fake, 8, 4, 2, None, fake, 0, None, None),
        lambda: lib.mjmpc_sample_noise_batch(_lib.F64, 4, fake, 8, 4, 2, fake, None, 0, None, None),
        lambda: lib.mjmpc_sample_noise_batch(_lib.F64, 0, fake, 8, 4, 2, fake, fake, 0, None, None),
        lambda: lib.mjmpc_sample_noise_batch(_lib.F64, 65536, fake, 8, 4, 2, fake, fake, 0, None, None),
        lambda: lib.mjmpc_sample_noise_batch(_lib.F64, 4, fake, 0, 4, 2, fake, fake, 0, None, None),
        lambda: lib.mjmpc_mppi_fused_update_batch(_lib.F64, 4, 64, 8, 2, None, fake, fake, fake, 0, fake, None, None, fake, None),
        lambda: lib.mjmpc_mppi_fused_update_batch(_lib.F64, 4, 64, 8, 2, fake, fake, None, fake, 0, fake, None, None, fake, None),
        lambda: lib.mjmpc_mppi_fused_update_batch(_lib.F64, 4, 64, 8, 2, fake, fake, fake, fake, 0, fake, None, None, None, None),
        lambda: lib.mjmpc_mppi_fused_update_batch(_lib.F64, 0, 64, 8, 2, fake, fake, fake, fake, 0, fake, None, None, fake, None),
        lambda: lib.mjmpc_mppi_fused_update_batch(_lib.F64, 70000, 64, 8, 2, fake, fake, fake, fake, 0, fake, None, None, fake, None),
        lambda: lib.mjmpc_mppi_fused_update_batch(_lib.F64, 4, 64, 8, 2, fake, fake, fake, fake, 2, fake, None, None, fake, None),
        lambda: lib.mjmpc_mppi_fused_update_batch(_lib.F64, 4, 0, 8, 2, fake, fake, fake, fake, 0, fake, None, None, fake, None),
        lambda: lib.mjmpc_update_batch_workspace_bytes(0, 64, 8, 2),
        lambda: lib.mjmpc_update_batch_workspace_bytes(65536, 64, 8, 2),
        lambda: lib.mjmpc_update_batch_workspace_bytes(4, 0, 8, 2),
    ]
    for i, call in enumerate(bad):
        lib.mjmpc_last_error()
        rc = call()
        assert rc != 0, i
        assert len(lib.mjmpc_last_error()) > 0, i
    # the workspace of E episodes is E single-episode partial blocks: ceil(P / 64) partials of 2 + H A doubles each
    assert lib.mjmpc_update_batch_workspace_bytes(4, 256, 16, 6) == 8 * 4 * 4 * (2 + 16 * 6)
    assert lib.mjmpc_update_batch_workspace_bytes(1, 65, 2, 1) == 8 * 2 * 4


def _kw(**over):
    kw = dict(raw_model=half_cheetah_raw(), num_episodes=4, horizon=8, num_particles=64, lam=0.2, step_size=1.0, init_cov=0.3,
              gamma=1.0, filter_coeffs=[0.25, 0.8, 0.0], base_action="null", seeds=[1, 2, 3, 4])
    kw.update(over)
    return kw


@pytest.mark.parametrize("over", bc.COMMON_REFUSED + [
    dict(use_zero_control_seq=True), dict(alpha=0), dict(time_based_weights=True), dict(cov_type="full"),
    # per-episode arrays of the wrong length / shape, and values MPPI cannot take
    dict(lam=[0.1, 0.2, 0.3]), dict(step_size=np.ones(5)), dict(init_cov=[0.1] * 3), dict(init_mean=np.zeros((3, 8, 6))),
    dict(init_mean=np.zeros((8, 5))), dict(lam=0.0), dict(init_cov=[0.3, 0.3, -1.0, 0.3]),
    dict(raw_model=bc.rk4_hand()),
], ids=bc.refused_id())
def test_unsupported_settings_raise_before_any_engine(no_engine, over):     # noqa: F811
    from mjmpc_amd.control import BatchedMPPI
    with pytest.raises(ValueError):
        BatchedMPPI(**_kw(**over))


def test_supported_settings_reach_the_engine(no_engine):                    # noqa: F811
    """The settings the batch runs pass the checks (and then get as far as making the engine)."""
    from mjmpc_amd.control import BatchedMPPI
    bc.check_reaches_the_engine(BatchedMPPI, [_kw(), _kw(
        lam=[0.1, 0.2, 0.3, 0.4], step_size=[1.0, 0.9, 0.8, 0.7], init_cov=[0.1, 0.2, 0.3, 0.4], base_action="repeat",
        dtype="f32", init_mean=np.zeros((4, 8, 6)), seeds=np.arange(4))])
