"""No GPU: the table of tests/points_tile_cases.py covers what tests/test_points_tiles_gpu.py is there for - every tile size of
the points launcher in both types under both entries, the edges of the widths and of N, the largest programs - and every case
passes the launcher's documented checks; the 80-bit interpreter agrees with the float64 one and, through it, with the C oracle
on the model cases; and the two criteria have teeth: the float64 interpreter (rounded once, for f32) passes them on every case,
float32 arithmetic and an interpreter with one documented mistake do not.

Measured over the table: max |interp64 - want80| 6.4e-17 .. 3.6e-13 per case, so bounds of 2.0e-15 .. 1.2e-11; the float32
interpreter misses the f32 criterion on the deep cases by 1.8e-5 and more, the wrong interpreters the f64 one by 2 and more."""
import numpy as np
import pytest

import motion_cases as mc
import points_cases as pc
import points_tile_cases as tc

LD = np.longdouble
COMBOS = [(d, e) for d in ("f64", "f32") for e in ("points", "motion")]


def _of(dtype, entry):
    return [c for c in tc.cases() if (c.dtype, c.entry) == (dtype, entry)]


# ---- the table ----------------------------------------------------------------------------------------------------------------
def test_the_tile_rule_restated():
    """Spot values worked out by hand from the launcher's rule: (rows word pitch, rounded up to 8) + 24 rows n_out <= 61440."""
    assert np.finfo(LD).eps < 2e-19                                     # 80-bit: what the bounds below rest on
    assert tc.tile_rows("f64", 23, 2) == 256 and tc.tile_rows("f64", 24, 2) == 128      # 256 (8 * 23 + 48) = 59392; pitch 25: 63488
    assert tc.tile_rows("f32", 47, 2) == 256 and tc.tile_rows("f32", 48, 2) == 128      # 256 (4 * 47 + 48) = 60416; pitch 49: 62464
    assert tc.tile_rows("f64", 7673, 1) == 1 and tc.widest("f64", 1) == 7675 and tc.tile_rows("f64", 7675, 1) == 1
    assert tc.tile_rows("f32", 64, 5) == 128 and tc.tile_rows("f32", 64, 16) == 64
    assert tc.widest("f32", 16) == 15261 and tc.widest("f64", 16) == 7630
    assert [tc.threads(r) for r in tc.TILES] == [256, 128, 64, 64, 64, 64, 64, 64, 64]


@pytest.mark.parametrize("dtype,entry", COMBOS)
def test_every_tile_size_and_every_edge_is_in_the_table(dtype, entry):
    mine = _of(dtype, entry)
    assert {tc.tile_rows(c.dtype, c.d_obs, c.n_out) for c in mine} == set(tc.TILES)
    tags = set()
    for c in mine:
        assert tc.refusal(c) is None, (c.name, tc.refusal(c))
        rows = tc.tile_rows(c.dtype, c.d_obs, c.n_out)
        wg = tc.threads(rows)
        assert rows == c.tile and c.obs.shape == (c.N, c.d_obs) and c.program.shape == (c.n_rows + c.n_diff, 16)
        assert c.obs.dtype == (np.float32 if dtype == "f32" else np.float64) and c.program.dtype == np.float64
        assert (c.dofadr is not None and c.dofadr.shape == (c.n_rows,) and c.dofadr.dtype == np.int32) == (entry == "motion")
        if "narrowest" in c.tags:                                       # no narrower row (behind qpos, qvel, the special words)
            assert c.d_obs == c.base + tc.PAD or tc.tile_rows(c.dtype, c.d_obs - 1, c.n_out) == 2 * rows
        for tag, holds in (("N = 1", c.N == 1), ("N = rows", c.N == rows), ("N = rows + 1", c.N == rows + 1),
                           ("ragged", c.N == 2 * rows + rows // 2 + 1), ("d_obs == wg", c.d_obs == wg),
                           ("d_obs a multiple of wg", c.d_obs % wg == 0 and c.d_obs > wg), ("d_obs > wg", c.d_obs > wg),
                           ("d_aug a multiple of wg", c.d_aug % wg == 0), ("even d_obs", c.d_obs % 2 == 0),
                           ("odd d_obs", c.d_obs % 2 == 1), ("dr == 0 in the copy out", c.d_aug > wg),
                           ("three workgroups of 256", rows == 256 and c.N > 512)):
            assert holds or tag not in c.tags, (c.name, tag)            # a tag the case carries is true of it
            if holds:
                tags.add((tag, rows) if tag.startswith(("N =", "ragged")) else tag)
        tags |= {t for t in c.tags if t in ("wild", "full", "shared") or "past" in t or "slot" in t or "difference" in t or "a ==" in t}
    assert {("ragged", r) for r in tc.TILES} <= tags                    # every tile size with a ragged last tile
    for r in (256, 64, 16, 2):
        assert {("N = 1", r), ("N = rows", r), ("N = rows + 1", r)} <= tags
    want = {"d_obs == wg", "d_obs a multiple of wg", "d_obs > wg", "d_aug a multiple of wg", "even d_obs", "odd d_obs",
            "dr == 0 in the copy out", "three workgroups of 256", "wild", "full", "ball past nq", "free past nq", "slot outside",
            "a == b", "difference index below 0", "difference index above n_out - 1"}
    if entry == "motion":
        want |= {"shared", "dof past nv", "difference of an unnamed slot"}
    assert want <= tags, want - tags


@pytest.mark.parametrize("dtype,entry", COMBOS)
def test_the_largest_programs(dtype, entry):
    deep = [c for c in _of(dtype, entry) if c.deep]
    assert [c.name.split("-")[-1] for c in deep] == (["full", "shared"] if entry == "motion" else ["full"])
    for c in deep:
        rows = c.program[:c.n_rows]
        node = np.isin(rows[:, 0], list(tc.NQ_OF))
        closing = np.flatnonzero(~node)
        assert (c.n_rows, c.n_out, c.n_diff, c.nodes) == (tc.MAX_ROWS, 16, 16, tc.MAX_NODES) == (544, 16, 16, 33)
        assert np.all(rows[node, 0] >= 1) and np.all(np.isin(rows[closing, 0], mc.CLOSING if entry == "motion" else (0,)))
        walks = np.split(np.arange(c.n_rows), closing[rows[closing, 1] == 0] + 1)[:-1]          # (keep is 0 under mjmpc_points)
        lengths = [int(node[w].sum()) for w in walks]
        assert len(walks) == 16 and max(lengths) == 33 and sum(lengths) + len(closing) == 544
        frees = np.flatnonzero(rows[:, 0] == tc.FREE)
        assert len(frees) == 1 and frees[0] == 0                        # one walk starts at a free joint; none holds one later
        assert all((rows[w, 0] == tc.BALL).sum() >= 4 for w in walks)   # several ball joints on every walk
        assert {tc.HINGE, tc.SLIDE, tc.BALL, tc.FREE} == set(rows[node, 0].astype(int))
        assert np.all(c.program[c.n_rows:, 0] == tc.DIFFERENCE)
        slots = rows[closing, 2].astype(int)
        if c.name.endswith("full"):
            assert lengths == [33] * 16 and len(closing) == 16 and np.any(c.program[c.n_rows:, 1] == c.program[c.n_rows:, 2])
            if entry == "motion":
                assert slots.tolist() == list(range(16)) and set(rows[closing, 0]) == set(mc.CLOSING)
            else:
                assert np.all(rows[closing, 1:3] == 0)
        else:
            shared = [w for w in walks if (~node[w]).sum() > 1]
            assert len(shared) == 1 and sorted(rows[shared[0]][~node[shared[0]], 0]) == sorted(mc.CLOSING)
            assert rows[shared[0]][~node[shared[0]], 1].tolist() == [1, 1, 1, 0]
            named = slots[(slots >= 0) & (slots < 16)]
            assert len(set(named)) == len(named) == 14 and np.any(np.diff(named) < 0)          # no slot twice; out of order
            unnamed = set(range(16)) - set(named)
            assert len(unnamed) >= 2 and np.any(np.isin(c.program[c.n_rows:, 1:3], list(unnamed)))
            assert np.any(slots < 0) and np.any(slots > 15)


def test_node_contents_and_inputs():
    """Orientations and axes are unit to float64 rounding, offsets and anchors around 0.1, qpos0 nonzero; hinge and slide entries
    reach pi about qpos0, qvel is of order 1, the quaternions of qpos come with norms 0.5, 1 and 3; f32 rows are f32 values."""
    norms = set()
    for c in tc.cases():
        rows = c.program[:c.n_rows]
        if "wild" in c.tags:
            continue
        for k, row in enumerate(rows):
            kind, adr = int(row[0]), int(row[1])
            if kind not in tc.NQ_OF:
                continue
            if kind != tc.FREE:
                assert abs(np.linalg.norm(row[6:10]) - 1.0) <= 4e-16 and 0.0499 < np.linalg.norm(row[3:6]) < 0.2001
            if kind in (tc.HINGE, tc.SLIDE):
                assert abs(np.linalg.norm(row[10:13]) - 1.0) <= 4e-16 and 0.2 <= abs(row[2]) <= 0.9
                d = c.obs[:, adr].astype(np.float64) - row[2]
                assert np.all(np.abs(d) <= np.pi + 1e-6) and (c.N < 40 or np.abs(d).max() > 2.0)
            if kind in (tc.HINGE, tc.BALL):
                assert 0.0499 < np.linalg.norm(row[13:16]) < 0.2001
            if kind in (tc.BALL, tc.FREE):
                q = c.obs[:, adr + (3 if kind == tc.FREE else 0):][:, :4].astype(np.float64)
                norms |= set(np.round(np.linalg.norm(q, axis=1), 3))
            if c.entry == "motion":
                assert 0 <= c.dofadr[k] and c.dofadr[k] + tc.NV_OF[kind] <= c.nv and adr + tc.NQ_OF[kind] <= c.nq
        if c.entry == "motion" and c.N >= 20:
            assert 0.5 < np.abs(c.obs[:, c.nq:c.nq + c.nv]).mean() < 1.2
    assert norms == {0.5, 1.0, 3.0}


@pytest.mark.parametrize("dtype,entry", COMBOS)
def test_the_copied_entries_hold_every_special_word(dtype, entry):
    for c in _of(dtype, entry):
        seen, nans = tc.special_classes(c)
        assert c.d_obs >= c.base + min(tc.PAD, 9), c.name
        if c.N >= tc.PAD or c.d_obs >= c.base + tc.PAD:
            assert seen == set(tc.SPECIAL_CLASSES) and nans >= 6, (c.name, seen, nans)
        else:
            assert len(seen) >= 3, (c.name, seen)


# ---- the 80-bit interpreter -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.case_names())
def test_the_80_bit_interpreters_on_the_model_cases(name):
    """Both interpreters in ``np.longdouble`` against their float64 selves and the C oracle at the bounds tests/test_points_cpu.py
    and tests/test_motion_cpu.py use; ``motion_cases.interpret`` reads a points-only program as ``points_cases.interpret`` does."""
    from test_motion_cpu import POSITION_BOUND, RATE_BOUND, _errors, _run as motion_run
    from test_points_cpu import _run as points_run
    raw, program, n_rows, states, got64, oracle = points_run(name)
    n_points = int(np.sum(program[:n_rows, 0] == pc.POINT))
    got80 = np.array([pc.interpret(program, n_rows, q, dtype=LD) for q in states])
    assert got80.dtype == LD and np.abs(got80 - got64).max() <= 1e-12 and np.abs(got80 - oracle).max() <= 1e-12
    assert 0 < np.abs(got80 - got64).max() < 1e-13                      # (it is not the float64 run again)
    as_motion = mc.interpret(program, n_rows, None, n_points, np.array(states), None, dtype=LD, slots_in_order=True)
    assert as_motion.dtype == LD and np.abs(as_motion - got80).max() <= 1e-17 * max(1.0, np.abs(got80).max()) * n_rows
    for guards in (False, True):                                        # on a sound table the guards change nothing
        again = mc.interpret(program, n_rows, None, n_points, np.array(states), None, slots_in_order=True, guards=guards)
        assert again.dtype == np.float64 and np.abs(again - got64).max() <= 1e-13
    assert np.array_equal(np.array([pc.interpret(program, n_rows, q, guards=True, n_points=n_points) for q in states]), got64)

    run = motion_run(name)
    program, n_rows, n_out, _, dofadr = run["table"]
    q, qd = np.array([s[0] for s in run["states"]]), np.array([s[1] for s in run["states"]])
    got80 = mc.interpret(program, n_rows, dofadr, n_out, q, qd, dtype=LD)
    guarded = np.array([mc.interpret(program, n_rows, dofadr, n_out, *s, guards=True) for s in run["states"]])
    assert got80.dtype == LD and np.array_equal(guarded, run["got"])    # on a sound table the guards change nothing
    position, rate = _errors(run, got80.astype(np.float64))
    assert position <= POSITION_BOUND and rate <= RATE_BOUND
    assert 0 < np.abs(got80 - run["got"]).max() <= 1e-11


def test_no_float64_on_the_value_path():
    """In float32 the interpreters return float32 and differ from the float64 run by float32's rounding: an intermediate held in
    float64 anywhere would have widened the result's type."""
    c = tc.case("motion-f32-t64")
    low = tc.interpret(c, np.float32)
    assert low.dtype == np.float32 and 1e-7 < np.abs(low - tc.reference(c.name)[1]).max() < 1e-3
    c = tc.case("points-f32-t64")
    low = np.array([pc.interpret(c.program, c.n_rows, q, dtype=np.float32, guards=True) for q in c.obs[:, :c.nq]])
    assert low.dtype == np.float32 and 1e-7 < np.abs(low - tc.reference(c.name)[1]).max() < 1e-3


@pytest.mark.parametrize("name", [c.name for c in tc.cases() if c.entry == "points" and "ragged" in c.tags and c.tile in (32, 64)])
def test_the_two_interpreters_agree_on_the_synthetic_points_programs(name):
    """points_cases' loop over one state and motion_cases' over a batch, both in 80-bit with the guards, wild tables included."""
    c = tc.case(name)
    want80 = tc.reference(name)[0]
    rows = range(0, c.N, 7)
    one = np.array([pc.interpret(c.program, c.n_rows, c.obs[n, :c.nq], dtype=LD, guards=True, n_points=c.n_out) for n in rows])
    assert np.abs(one - want80[::7]).max() <= 64 * np.finfo(LD).eps * c.nodes * max(1.0, float(np.abs(want80).max()))


# ---- the criteria ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tc.names())
def test_the_float64_interpreter_passes_both_criteria(name):
    c = tc.case(name)
    want80, interp64, bound = tc.reference(name)
    floor = (c.nodes + 2) * 2.0 ** -52 * max(1.0, float(np.abs(want80).max()))
    own = float(np.abs(interp64 - want80).max())
    assert bound == max(32 * own, floor) and 0 < own < 1e-12
    assert tc.excess_f64(interp64, want80, bound)[0] <= 0.0
    excess, worst, ulps = tc.excess_f32(interp64.astype(np.float32), want80, bound)
    assert excess <= 0.0 and ulps <= 0.5 + 1e-5
    assert worst > 1e-9 or np.abs(want80).max() < 0.1                   # (half an ulp is most of the f32 criterion)


@pytest.mark.parametrize("name", [c.name for c in tc.cases() if c.deep])
def test_the_criteria_fail_what_is_wrong(name):
    c = tc.case(name)
    want80, interp64, bound = tc.reference(name)
    # float32 arithmetic from the same rows: no longer "computed in double, rounded once"
    low = tc.interpret(c, np.float32)
    assert low.dtype == np.float32
    excess, _, ulps = tc.excess_f32(low, want80, bound)
    print("%s: float32 arithmetic misses the f32 criterion by %.3g (%.0f ulp32)" % (name, excess, ulps))
    assert excess > 1e3 * bound and ulps > 8
    # one documented mistake: the hinge's anchor dropped (positions), its lever arm dropped (velocities)
    for wrong in ("anchor", "hinge_lever"):
        excess, worst = tc.excess_f64(tc.interpret(c, np.float64, wrong=wrong), want80, bound)
        print("%s: wrong=%r misses the f64 criterion by %.3g" % (name, wrong, excess))
        if wrong == "anchor" or c.entry == "motion":
            assert excess > 1e-3 and excess > 1e6 * bound
        else:
            assert excess <= 0.0                                        # (no velocity among mjmpc_points' outputs)
