"""GPU: ``MPPIQ(alpha=1, noise_mode='device')`` runs as a captured closed loop (``enable_graph(post_step=engine.step_state)``),
because ``DeviceUpdater.td_lambda_returns`` keeps its weight table on the device.  HalfCheetah on the tree engine, P = 48, H = 8,
T = 3, f64."""
import numpy as np
import pytest

from batched_cases import FILT, _cheetah_states, _torch
from batched_cases import cheetah as _cheetah

pytestmark = pytest.mark.gpu

P, H, T, SEED = 48, 8, 3, 123


def _controller(eng, alpha=1):
    from mjmpc_amd.control import MPPIQ
    from mjmpc_amd.envs.arm_engine import make_device_rollout_fn
    c = MPPIQ(d_state=eng.d_state, d_obs=eng.d_obs, d_action=eng.d_action, horizon=H, base_action="null", num_particles=P,
              gamma=1.0, n_iters=1, action_lows=eng.action_lows, action_highs=eng.action_highs, filter_coeffs=FILT, seed=SEED,
              noise_mode="device", noise_dtype="f64", init_cov=0.3, beta=0.2, step_size=0.8, alpha=alpha, td_lam=0.9,
              time_based_weights=True)
    c.rollout_fn = make_device_rollout_fn(eng)
    c.set_sim_state_fn = lambda s: None
    return c


def _loop(captured, count=None):
    """T steps of the closed loop -> actions [T][A], the final mean, the final state."""
    torch = _torch()
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    eng = TreeRolloutEngine(_cheetah(), dtype="f64")
    eng.set_env_state(dict(_cheetah_states(1)[0]))
    c = _controller(eng)
    if captured:
        c.enable_graph(post_step=eng.step_state)
    acts = []
    for t in range(T):
        if count is not None:
            count.append(0)
        a, _ = c.optimize(None)
        a = np.array(a, np.float64)
        if not captured:
            eng.step_state(torch.from_numpy(a.copy()).to("cuda"))
        torch.cuda.synchronize()
        acts.append(a)
    if captured:
        assert c._graph is not None and not getattr(c, "graph_fallback", False)        # (it did replay a capture)
    out = np.array(acts), np.array(c.mean_action), eng.get_state_device()
    assert eng.env_resets() == 0
    eng.close()
    return out


def test_captured_loop_equals_the_eager_loop():
    acts_g, mean_g, state_g = _loop(True)
    acts_e, mean_e, state_e = _loop(False)
    assert np.all(np.isfinite(acts_e)) and np.any(acts_e != 0)
    assert np.array_equal(acts_g, acts_e), "actions differ (max %.3g)" % np.abs(acts_g - acts_e).max()
    assert np.array_equal(mean_g, mean_e)
    for k in state_e:
        assert np.array_equal(state_g[k], state_e[k]), k


def test_returns_upload_nothing_from_their_second_step_on(monkeypatch):
    """The weight table goes up once; from the second step on ``td_lambda_returns`` copies nothing from the host (counted at the
    upload helper, not timed)."""
    from mjmpc_amd.control._device import DeviceUpdater
    count = []
    real = DeviceUpdater._upload

    def counting(self, dst, host):
        count[-1] += 1
        return real(self, dst, host)
    monkeypatch.setattr(DeviceUpdater, "_upload", counting)
    _loop(False, count)
    assert count == [1] + [0] * (T - 1)


def test_control_cost_still_refuses_capture():
    """alpha = 0 uploads cov^-1 on every update: ``enable_graph`` refuses instead of failing inside the capture."""
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    eng = TreeRolloutEngine(_cheetah(), dtype="f64")
    c = _controller(eng, alpha=0)
    assert c._host_uploads_per_step()
    with pytest.raises(ValueError, match="captured graph"):
        c.enable_graph(post_step=eng.step_state)
    eng.close()
    eng = TreeRolloutEngine(_cheetah(), dtype="f64")
    c = _controller(eng, alpha=1)
    assert not c._host_uploads_per_step()
    c.enable_graph(post_step=eng.step_state)
    eng.close()
