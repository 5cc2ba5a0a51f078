"""GPU: the softmax episode batches stay inside the workspace their size functions report.

``mjmpc_dmd_update_batch`` and ``mjmpc_mppiq_update_batch`` share one row layout (``SoftmaxRow``).  Each call runs twice on the
same random inputs: on a workspace of ``nbytes / 8 + 64`` doubles filled with NaN, and on a zero-filled workspace of exactly
``nbytes``.  The 64 trailing doubles must keep their NaN bit pattern (nothing is written past ``*_batch_workspace_bytes``), the
results must be finite (no cell is read before it is written) and the two runs must agree with ``np.array_equal``.  The rows
are compared with the single-episode path in ``test_batched_dmd_gpu.py`` and ``test_batched_mppiq_gpu.py``.
"""
import ctypes

import numpy as np
import pytest

from batched_cases import _torch, _vp

pytestmark = pytest.mark.gpu

E, P, A, TAIL = 2, 17, 2, 64            # P = 17: one full chunk of 16 particles and a ragged one
NAN_BITS = np.array(np.nan).view(np.int64)


def _run_twice(nbytes, call, outputs):
    """call(ws) on the NaN-filled oversized workspace, then on the zero-filled exact one; outputs() -> host copies of the results
    after either.  Returns both sets of results and the trailing doubles of the first workspace, as bit patterns."""
    torch = _torch()
    assert nbytes > 0 and nbytes % 8 == 0
    ws = torch.full((nbytes // 8 + TAIL,), float("nan"), dtype=torch.float64, device="cuda")
    call(ws)
    torch.cuda.synchronize()
    padded, tail = outputs(), ws[nbytes // 8:].cpu().numpy().view(np.int64)
    call(torch.zeros(nbytes // 8, dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    return padded, outputs(), tail


def _check(padded, exact, tail):
    assert tail.shape == (TAIL,) and np.all(tail == NAN_BITS), "written past the reported workspace size"
    for k in padded:
        assert np.all(np.isfinite(padded[k])), "%s: a workspace cell was read before it was written" % k
        assert np.array_equal(padded[k], exact[k]), k


def _dev(a, dt=None):
    torch = _torch()
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    return t if dt is None else t.to(dt)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("H", [3, 1])
@pytest.mark.parametrize("cov_mode", [1, 2])
def test_dmd_update_batch_stays_inside_its_workspace(cov_mode, H, dtype):
    torch = _torch()
    from mjmpc_amd import _lib
    lib = _lib.require_gpu()
    code, tdt = (_lib.F32, torch.float32) if dtype == "f32" else (_lib.F64, torch.float64)
    rng = np.random.RandomState(17 + 10 * H)
    costs, actions = rng.uniform(0.0, 2.0, (E, P, H)), rng.uniform(-1, 1, (E, P, H, A))
    means0 = rng.uniform(-0.2, 0.2, (E, H, A))
    m = rng.uniform(-1, 1, (E, A, A))
    covs0 = 0.3 * (m @ m.transpose(0, 2, 1) / A + 0.5 * np.eye(A))
    d_costs, d_act, d_gseq = _dev(costs, tdt), _dev(actions, tdt), _dev(np.cumprod([1.0] + [0.97] * (H - 1)))
    d_lam, d_step, d_beta = _dev(np.array([0.2, 1.0])), _dev(np.array([1.0, 0.7])), _dev(np.array([0.05, 0.3]))
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    b = {}

    def call(ws):
        b.update(means=_dev(means0), covs=_dev(covs0), out=torch.zeros((E, A), dtype=torch.float64, device="cuda"),
                 counter=torch.zeros(1, dtype=torch.int64, device="cuda"))
        _lib.check(lib.mjmpc_dmd_update_batch(code, E, P, H, A, _vp(d_costs), _vp(d_act), _vp(d_gseq), _vp(d_lam), _vp(d_step),
                                              cov_mode, _vp(d_beta), 0, _vp(b["means"]), _vp(b["covs"]), _vp(b["out"]),
                                              _vp(b["counter"]), _vp(ws), s))

    _check(*_run_twice(lib.mjmpc_dmd_batch_workspace_bytes(E, P, H, A), call, lambda: {k: v.cpu().numpy() for k, v in b.items()}))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("H", [3, 1])
@pytest.mark.parametrize("alpha", [0, 1])
@pytest.mark.parametrize("tbw", [0, 1])
def test_mppiq_update_batch_stays_inside_its_workspace(tbw, alpha, H, dtype):
    torch = _torch()
    from mjmpc_amd import _lib
    lib = _lib.require_gpu()
    code, npt = (_lib.F32, np.float32) if dtype == "f32" else (_lib.F64, np.float64)
    rs = np.random.RandomState(8 + H)
    td_lam, gamma = np.array([0.85, 0.0]), 0.97
    means0 = 0.2 * rs.randn(E, H, A)
    actions = (means0[:, None] + 0.5 * rs.randn(E, P, H, A)).astype(npt)
    costs = (rs.rand(E, P, H) * 2).astype(npt)
    wseq = np.stack([np.cumprod([1.0] + [gamma * l] * (H - 2)) if H > 1 else np.array([1.0]) for l in td_lam])
    wzero = np.array([int(bool(np.any(w == 0))) for w in wseq], np.int32)
    covinv = np.stack([np.linalg.inv(np.diag(np.full(A, c))) for c in (0.9, 0.5)])
    d_costs, d_act, d_beta, d_step, d_tdl, d_wseq, d_wz, d_cinv = (
        _dev(x) for x in (costs, actions, np.array([0.4, 0.15]), np.array([0.8, 1.0]), td_lam, wseq, wzero, covinv))
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    b = {}

    def call(ws):
        b.update(means=_dev(means0), out=torch.zeros((E, A), dtype=torch.float64, device="cuda"),
                 counter=torch.zeros(1, dtype=torch.int64, device="cuda"))
        _lib.check(lib.mjmpc_mppiq_update_batch(code, E, P, H, A, _vp(d_costs), _vp(d_act), _vp(d_beta), _vp(d_step), _vp(d_tdl),
                                                _vp(d_wseq), _vp(d_wz), gamma, alpha, _vp(d_cinv) if alpha == 0 else None, tbw, 0,
                                                _vp(b["means"]), _vp(b["out"]), _vp(b["counter"]), _vp(ws), s))

    _check(*_run_twice(lib.mjmpc_mppiq_batch_workspace_bytes(E, P, H, A, tbw), call,
                       lambda: {k: v.cpu().numpy() for k, v in b.items()}))
