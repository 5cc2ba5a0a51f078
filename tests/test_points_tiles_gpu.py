"""GPU: ``mjmpc_points`` and ``mjmpc_points_motion`` at the C entries over tests/points_tile_cases.py - every tile size of the
launcher (256 .. 1 rows; below 64 rows a workgroup keeps 64 threads), d_obs at, above and a multiple of the thread count, ragged
last tiles, the largest programs the header allows, the kernel's guards - each case one launch with canary rows on both sides of
the output, held to the numpy interpreter of tests/motion_cases.py run in 80-bit ``np.longdouble`` over the same rows:

  f64   |got - want80| <= bound(case) = 32 max |interp64 - want80| over the case, no less than (nodes + 2) 2^-52 max(1, |want80|)
  f32   |got - want80| <= ulp32(want80) / 2 + bound(case): "computed in double, rounded once" (want80 from the widened f32 rows)

and the copied observation - signed zeros, infinities, denormals, NaNs with payloads among it - compared as integers.
tests/test_points_tiles_cpu.py shows that the float64 interpreter passes both criteria and what fails them.

Measured on an MI355X (each case prints its own line; the table: profiles/r28_points_tiles.txt): over the 55 f64 cases the
kernel's worst error is 0.44 to 3.2 times the float64 interpreter's own and at most 0.10 of the bound (1.5e-13 absolute at worst,
motion-f64-shared, entries up to 80); over the 55 f32 cases it is never above 0.5000 ulp32, and all 154359 new entries equal
``np.float32`` of the f64 entry's launch over the widened rows bit for bit (reported, not asserted).  A kernel that rounds a
difference's operands before it subtracts them fails 54 of the f32 cases."""
import ctypes

import numpy as np
import pytest

import points_tile_cases as tc

pytestmark = pytest.mark.gpu

CANARY = 7.0
_RAN = {}


def _launch(c, dtype, obs):
    """One launch of the case's entry over ``obs`` [N][d_obs] in ``dtype``; -> the output [N + 2][d_aug], canary rows first and
    last."""
    import torch
    from mjmpc_amd import _lib
    lib = _lib.require_gpu()
    assert tc.refusal(c) is None and obs.shape == (c.N, c.d_obs)
    if dtype == c.dtype:
        assert tc.tile_rows(dtype, c.d_obs, c.n_out) == c.tile                     # the tile this launch takes is the table's
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    obs_d, prog_d = torch.from_numpy(obs).cuda(), torch.from_numpy(c.program).cuda()
    out = torch.full((c.N + 2, c.d_aug), CANARY, dtype=obs_d.dtype, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    code = _lib.F32 if dtype == "f32" else _lib.F64
    if c.entry == "motion":
        dof_d = torch.from_numpy(c.dofadr).cuda()
        _lib.check(lib.mjmpc_points_motion(code, c.N, c.d_obs, c.nq, c.nv, vp(obs_d), vp(prog_d), vp(dof_d), c.n_rows, c.n_out,
                                           c.n_diff, vp(out[1:]), stream))
    else:
        _lib.check(lib.mjmpc_points(code, c.N, c.d_obs, c.nq, vp(obs_d), vp(prog_d), c.n_rows, c.n_out, c.n_diff, vp(out[1:]),
                                    stream))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _run(name):
    c = tc.case(name)
    want80, interp64, bound = tc.reference(name)
    f32 = c.dtype == "f32"
    got = _launch(c, c.dtype, c.obs)
    assert got.dtype == c.obs.dtype == (np.float32 if f32 else np.float64)
    assert np.all(got[0] == CANARY) and np.all(got[-1] == CANARY)                   # nothing written before or behind
    got = got[1:-1]
    bits = np.uint32 if f32 else np.uint64
    assert np.array_equal(got[:, :c.d_obs].view(bits), c.obs.view(bits))            # the observation, bit for bit
    new = got[:, c.d_obs:]
    assert new.shape == want80.shape
    excess, worst, *ulps = (tc.excess_f32 if f32 else tc.excess_f64)(new, want80, bound)
    own = float(np.abs(interp64.astype(np.longdouble) - want80).max())
    line = "%-36s tile %3d  wg %3d  N %3d  d_obs %4d  rows %3d  worst |kernel - want80| %.3g  interp64's %.3g  bound %.3g" \
        % (name, c.tile, tc.threads(c.tile), c.N, c.d_obs, c.n_rows, worst, own, bound)
    if f32:
        # the f64 entry over the same values, widened: how many f32 entries are its entries rounded once (reported only)
        with np.errstate(invalid="ignore"):     # (the signalling NaNs among the copied entries)
            widened = c.obs.astype(np.float64)
        wide = _launch(c, "f64", widened)[1:-1, c.d_obs:]
        same = int(np.sum(wide.astype(np.float32).view(np.uint32) == new.view(np.uint32)))
        line += "  = %.4f ulp32  == float32(f64 launch) %d of %d" % (ulps[0], same, new.size)
        _RAN[name] = (c.dtype, c.entry, c.tile, same, new.size)
    else:
        _RAN[name] = (c.dtype, c.entry, c.tile, 0, 0)
    print(line)
    assert np.all(np.isfinite(new)) and excess <= 0.0, line


@pytest.mark.parametrize("name", tc.names())
def test_one_launch_against_the_80_bit_interpreter(name):
    _run(name)


def test_every_tile_size_ran_in_both_types_under_both_entries():
    for name in tc.names():                     # (all of them have, when the whole module runs)
        if name not in _RAN:
            _run(name)
    ran = {r[:3] for r in _RAN.values()}
    assert ran >= {(d, e, t) for d in ("f64", "f32") for e in ("points", "motion") for t in tc.TILES}
    same, size = sum(r[3] for r in _RAN.values()), sum(r[4] for r in _RAN.values())
    print("f32 entries equal to float32 of the f64 launch bit for bit: %d of %d" % (same, size))
