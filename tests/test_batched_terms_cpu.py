"""CPU: user-defined cost terms in the episode batches - the three entry points, every argument refusal of
theirs (a code and a message, nothing launched), what ``_EpisodeBatch.set_cost_terms`` refuses on the host, the per-episode
tables it builds, and a config block whose weights and targets list one value per episode."""
import numpy as np
import pytest

import batched_cases as bc
from mjmpc_amd import _lib
from mjmpc_amd.control import (BatchedCEM, BatchedDMDMPC, BatchedMPPI, BatchedMPPIQ, BatchedPFMPC, BatchedRandomShooting)
from mjmpc_amd.envs.arm_engine import ArmRolloutEngine
from mjmpc_amd.envs.cost_terms import CostTerms, cost_terms_from_config
from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
from mjmpc_amd.models.reacher7dof import reacher7dof_raw
from mjmpc_amd.models.synthetic import synthetic_raw

ENTRY_POINTS = ["mjmpc_tree_rollout_fused_batch_obs", "mjmpc_arm_rollout_fused_batch_obs", "mjmpc_cost_terms_batch"]
CLASSES = [BatchedMPPI, BatchedCEM, BatchedPFMPC, BatchedDMDMPC, BatchedRandomShooting, BatchedMPPIQ]


class _Device:      # (any call into the library or the device fails the test)
    def __getattr__(self, name):
        raise AssertionError("the device was reached: %s" % name)


@pytest.fixture(scope="module")
def cartpole():
    return TreeRolloutEngine.host_only(synthetic_raw("cartpole"))


@pytest.fixture(scope="module")
def reacher():
    return ArmRolloutEngine.host_only(reacher7dof_raw())


def _batch(cls, engine, E):
    """A batch with no device: what ``set_cost_terms`` reads before its first device call."""
    b = cls.__new__(cls)
    b.engine, b.num_episodes = engine, E
    b.lib = b.torch = _Device()
    return b


def test_entry_points_are_declared_bound_and_exported():
    bc.check_entry_points(ENTRY_POINTS, abi=4)


def test_rollout_entries_refuse_before_any_launch():
    lib = _lib.load()
    p = 64          # (never dereferenced: each call below fails its argument checks first)
    for fn in (lib.mjmpc_tree_rollout_fused_batch_obs, lib.mjmpc_arm_rollout_fused_batch_obs):
        for call in (lambda: fn(None, _lib.F64, 64, 8, p, p, None, None, p, p, None, p, None),      # null handle
                     lambda: fn(None, _lib.F64, 64, 8, p, p, None, None, p, p, None, None, None)):  # ... and no observations
            assert call() != 0
            assert len(lib.mjmpc_last_error()) > 0


def test_cost_terms_batch_bad_arguments_are_codes_and_messages():
    lib = _lib.load()
    p = 64          # (never dereferenced)
    f = lib.mjmpc_cost_terms_batch
    bad = [
        lambda: f(_lib.F64, 2, 4, 2, 3, 1, None, p, p, 1, 0, 0, 0, p, None, None, None),         # null observations
        lambda: f(_lib.F64, 2, 4, 2, 3, 1, p, p, None, 1, 0, 0, 0, p, None, None, None),         # null table
        lambda: f(_lib.F64, 2, 4, 2, 3, 1, p, p, p, 1, 0, 0, 0, None, None, None, None),         # null costs
        lambda: f(_lib.F64, 0, 4, 2, 3, 1, p, p, p, 1, 0, 0, 0, p, None, None, None),            # E < 1
        lambda: f(_lib.F64, 2, 0, 2, 3, 1, p, p, p, 1, 0, 0, 0, p, None, None, None),            # P < 1
        lambda: f(_lib.F64, 2, 4, 0, 3, 1, p, p, p, 1, 0, 0, 0, p, None, None, None),            # H < 1
        lambda: f(_lib.F64, 2, 4, 2, 0, 1, p, p, p, 1, 0, 0, 0, p, None, None, None),            # d_obs < 1
        lambda: f(_lib.F64, 2, 4, 2, 3, -1, p, None, p, 1, 0, 0, 0, p, None, None, None),        # A < 0
        lambda: f(_lib.F64, 2, 4, 2, 3, 0, p, p, p, 1, 0, 0, 0, p, None, None, None),            # actions with A < 1
        lambda: f(_lib.F64, 2, 4, 2, 3, 1, p, p, p, 0, 0, 0, 0, p, None, None, None),            # n_terms < 1
        lambda: f(_lib.F64, 2, 4, 2, 3, 1, p, p, p, 129, 0, 0, 0, p, None, None, None),          # n_terms > 128
        lambda: f(7, 2, 4, 2, 3, 1, p, p, p, 1, 0, 0, 0, p, None, None, None),                   # unknown dtype
        lambda: f(_lib.F64, 2, 4, 2, 3, 1, p, p, p, 1, 0, 0, 0, p, p, None, None),               # d_gseq without d_q0
        lambda: f(_lib.F64, 2, 4, 2, 3, 1, p, p, p, 1, 0, 0, 0, p, None, p, None),               # d_q0 without d_gseq
        lambda: f(_lib.F64, 2, 4, 2, 8000, 1, p, p, p, 1, 0, 0, 0, p, None, None, None),         # a row beyond the LDS tile
        lambda: f(_lib.F32, 2, 4, 2, 15000, 1, p, p, p, 1, 0, 0, 0, p, None, None, None),        # ... in f32
    ]
    for i, call in enumerate(bad):
        assert call() == -1, i                      # MJMPC_E_BADARG
        assert lib.mjmpc_last_error().startswith(b"mjmpc_cost_terms_batch"), (i, lib.mjmpc_last_error())


def _terms(engine, weight=1.0, target=0.0, keep=False):
    t = CostTerms(engine, keep_builtin=keep)
    t.abs(obs="site_minus_target", index=0, weight=weight)
    t.norm(obs="site_minus_target", weight=2.0, target=target)
    t.square(action=0, weight=0.1, terminal=True)
    return t


@pytest.mark.parametrize("cls", CLASSES, ids=lambda c: c.__name__)
def test_set_cost_terms_refusals_come_before_the_device(cls, cartpole):
    b = _batch(cls, cartpole, 3)
    good = _terms(cartpole)
    other_rows = _terms(cartpole).square(obs="qvel")
    other_kind = CostTerms(cartpole).square(obs="site_minus_target", index=0).norm(obs="site_minus_target", weight=2.0) \
        .square(action=0, weight=0.1, terminal=True)
    other_index = CostTerms(cartpole).abs(obs="site_minus_target", index=1).norm(obs="site_minus_target", weight=2.0) \
        .square(action=0, weight=0.1, terminal=True)
    other_when = CostTerms(cartpole).abs(obs="site_minus_target", index=0).norm(obs="site_minus_target", weight=2.0) \
        .square(action=0, weight=0.1)
    # (two norms over the halves of the block: the same kinds and indices, another grouping)
    one_group = CostTerms(cartpole).norm(obs="site_minus_target", index=[0, 1])
    two_groups = CostTerms(cartpole).norm(obs="site_minus_target", index=0).norm(obs="site_minus_target", index=1)
    outside = CostTerms().abs(obs=[cartpole.model.d_obs])       # (resolved against the engine only by set_cost_terms)
    for bad, match in [
        ([good, good], "one per episode"),                      # a list of the wrong length
        ([good] * 4, "one per episode"),
        ([good, other_rows, good], "rows"),                     # differing row counts
        ([good, other_kind, good], "kind"),                     # differing kind / index / when / group
        ([good, good, other_index], "index"),
        ([good, other_when, good], "when"),
        ([one_group, two_groups, one_group], "group"),
        ([good, _terms(cartpole, keep=True), good], "keep_builtin"),
        (CostTerms(cartpole), "empty"),                         # an empty table
        ([good, CostTerms(cartpole), good], "empty"),
        (outside, "outside"),                                   # an index outside the observation
        ([good, good, outside], "outside"),
        ("terms", "CostTerms"),
        ([good, None, good], "CostTerms"),
    ]:
        with pytest.raises(ValueError, match=match):
            b.set_cost_terms(bad)
    assert b._terms is None and b._terms_nobs is None
    b.set_cost_terms(None)                                      # (nothing set, nothing to restore: no device either)
    assert b.obs_layout() == cartpole.obs_layout()


def test_per_episode_tables_against_hand_written_rows(cartpole, reacher):
    lay = cartpole.obs_layout()["site_minus_target"]
    s = lay.start
    each = [_terms(cartpole, weight=w, target=t) for w, t in ((1.0, 0.0), (0.5, [0.1, 0.2, 0.3]), (-2.0, 0.25))]
    tables, keep, reads = BatchedMPPI._resolve_cost_terms(each, cartpole, 3)
    assert tables.shape == (3, 5, 8) and tables.dtype == np.float64 and keep is False and reads is True

    def rows(w, t):     # kind, source, index, weight, target, group, when, reserved
        return [[0, 0, s, w, 0.0, 0, 0, 0],
                [2, 0, s, 2.0, t[0], 1, 0, 0], [2, 0, s + 1, 2.0, t[1], 1, 0, 0], [2, 0, s + 2, 2.0, t[2], 1, 0, 0],
                [1, 1, 0, 0.1, 0.0, 0, 1, 0]]
    want = np.array([rows(1.0, [0.0] * 3), rows(0.5, [0.1, 0.2, 0.3]), rows(-2.0, [0.25] * 3)], np.float64)
    assert np.array_equal(tables, want)
    # one CostTerms: one table for every episode; no row reads an action
    t = CostTerms(reacher, keep_builtin=True).square(obs="qvel", weight=0.01)
    tables, keep, reads = BatchedCEM._resolve_cost_terms(t, reacher, 4)
    assert tables.shape == (1, 7, 8) and keep is True and reads is False
    assert np.array_equal(tables[0], t.table())
    # a list of one for a batch of one episode is a per-episode table of one
    assert BatchedMPPI._resolve_cost_terms([t], reacher, 1)[0].shape == (1, 7, 8)


def test_config_block_with_one_value_per_episode(cartpole):
    block = dict(keep_builtin=True, terms=[
        dict(kind="cos", obs="qpos", index=1, weight=4.0),
        dict(kind="square", obs="qpos", index=0, weight=0.5, target=[-0.4, 0.0, 0.4]),
        dict(kind="square", action=0, weight=[0.001, 0.01, 0.1]),
        dict(kind="norm", obs="site_minus_target", index=[0, 2], target=[[0.1, 0.2], [0.3, 0.4], [0.5, 0.6]]),
        dict(kind="abs", obs="qvel", target=[0.5, -0.5], terminal=True),       # (two entries: one per index, not per episode)
    ])
    each = cost_terms_from_config(block, cartpole, num_episodes=3)
    assert isinstance(each, list) and len(each) == 3 and all(t.keep_builtin for t in each)
    tables, keep, reads = BatchedMPPI._resolve_cost_terms(each, cartpole, 3)
    assert tables.shape == (3, 7, 8) and keep and reads
    assert tables[:, 1, 4].tolist() == [-0.4, 0.0, 0.4] and np.all(tables[:, 1, 3] == 0.5)
    assert tables[:, 2, 3].tolist() == [0.001, 0.01, 0.1]
    assert tables[:, 3:5, 4].tolist() == [[0.1, 0.2], [0.3, 0.4], [0.5, 0.6]]
    assert np.all(tables[:, 5:, 4] == [0.5, -0.5]) and np.all(tables[:, 5:, 6] == 1)
    # without per-episode lists: one CostTerms, with or without num_episodes; and the single-episode reading is unchanged
    shared = dict(terms=block["terms"][:1] + block["terms"][4:])
    one = cost_terms_from_config(shared, cartpole, num_episodes=3)
    assert isinstance(one, CostTerms) and np.array_equal(one.table(), cost_terms_from_config(shared, cartpole).table())
    with pytest.raises(ValueError, match="per episode"):
        cost_terms_from_config(dict(terms=[dict(kind="abs", obs="qvel", weight=[1.0, 2.0])]), cartpole, num_episodes=3)
    with pytest.raises(ValueError, match="per episode"):
        cost_terms_from_config(dict(terms=[dict(kind="abs", obs="qvel", weight=[1.0, 2.0])]), cartpole)


def test_the_batch_config_resolves_for_its_episodes(cartpole):
    import os
    import yaml
    with open(os.path.join(bc.ROOT, "examples", "configs", "cartpole_terms_batch_gpu.yml")) as f:
        exp = yaml.safe_load(f)
    each = cost_terms_from_config(exp["cost_terms"], cartpole, num_episodes=exp["n_episodes"])
    tables, keep, reads = BatchedMPPI._resolve_cost_terms(each, cartpole, exp["n_episodes"])
    assert tables.shape[0] == exp["n_episodes"] == 4 and not keep and reads
    assert len(set(tables[:, 1, 4])) == 4 and len(set(tables[:, 4, 3])) == 4
