"""No GPU: body axes and velocities in the cost terms - ``CostTerms.axis`` / ``velocity`` /
``angular_velocity`` build the motion program, the numpy interpreter of tests/motion_cases.py (written from the documented row
format) runs it, and the C oracle says what it must give: positions and axes from its kinematics (bound 1e-12), velocities and
angular velocities as the fourth-order central difference of those along ``qpos`` integrated by ``qvel`` with MuJoCo's rule
(``motion_cases.integrate`` restates it), ``h = 2.5e-4``, ``qvel ~ 2 N(0, 1)``.

Measured over the eight cases, 8 states each: positions and axes 1.0e-15 at worst; velocities and angular velocities against
the difference quotient 1.08e-10 at worst (random17; the five fixed models at or below 9.1e-12).  The bound on them is ten times
that, 1.08e-9; a convention error is of the order of the velocity itself, 0.1 to 6 here (the four wrong variants miss by 0.8 or
more)."""
import os

import numpy as np
import pytest

import motion_cases as mc
import points_cases as pc

N_STATES = 8
POSITION_BOUND = 1e-12
RATE_BOUND = 1.08e-9            # ten times the measured worst (the module's docstring); the issue's cap is 1e-6


def _terms(name):
    from mjmpc_amd.envs.cost_terms import CostTerms
    raw, kind, outputs, differences = mc.case(name)
    eng = pc.host_engine(raw, kind)
    return raw, eng, mc.add_outputs(CostTerms(eng), outputs, differences), outputs, differences


_RUNS = {}


def _run(name):
    """The case's program over its random states, made once: dict(raw, table, states, got, want, rate) - ``rate``: which entries
    are velocities or angular velocities (or differences of them)."""
    if name not in _RUNS:
        raw, eng, terms, outputs, differences = _terms(name)
        table = terms.points_table()
        program, n_rows, n_out, n_diff, dofadr = table
        assert (n_out, n_diff) == (len(outputs), len(differences)) and program.shape == (n_rows + n_diff, 16)
        assert dofadr.shape == (n_rows,) and dofadr.dtype == np.int32
        oracle = mc.Oracle(raw, *mc.resolved(raw, outputs, differences))
        rs = np.random.RandomState(23)
        states = [(pc.random_qpos(raw, rs), mc.random_qvel(raw, rs)) for _ in range(N_STATES)]
        rate = np.repeat([k in (mc.VELOCITY, mc.ANGULAR) for k in mc.kinds_of(outputs, differences)], 3)
        _RUNS[name] = dict(raw=raw, table=table, states=states, rate=rate,
                           got=np.array([mc.interpret(program, n_rows, dofadr, n_out, q, qd) for q, qd in states]),
                           want=np.array([oracle(q, qd) for q, qd in states]))
    return _RUNS[name]


def _errors(run, got=None):
    err = np.abs((run["got"] if got is None else got) - run["want"])
    return err[:, ~run["rate"]].max(), err[:, run["rate"]].max()


@pytest.mark.parametrize("name", mc.case_names())
def test_interpreted_program_matches_the_oracle(name):
    run = _run(name)
    assert N_STATES >= 6 and np.all(np.isfinite(run["want"]))
    position, rate = _errors(run)
    print("%s: %d rows, worst |interpreted - oracle| positions and axes %.3g, velocities %.3g"
          % (name, len(run["table"][0]), position, rate))
    assert position <= POSITION_BOUND
    assert rate <= RATE_BOUND <= 1e-6
    # liveness: qvel is of order 1 and every output moves or is moving
    assert 0.5 < np.mean([np.abs(qd).mean() for _, qd in run["states"]]) < 4.0
    # (but the axes and the angular velocity of a body behind slides alone: the cart-pole's cart)
    from mjmpc_amd.models.raw import JOINT_SLIDE
    blocks = run["got"].reshape(N_STATES, -1, 3)
    res, diffs = mc.resolved(run["raw"], *mc.case(name)[2:])
    fixed = [kind in (mc.AXIS, mc.ANGULAR) and all(run["raw"].bodies[b].joint is None or run["raw"].bodies[b].joint.type == JOINT_SLIDE
                                                   for b in pc.path(run["raw"], body)) for kind, body, _ in res]
    assert sum(fixed) <= 2 and (name == "cartpole" or not any(fixed))
    live = [not f for f in fixed] + [not (fixed[a] and fixed[b]) for a, b in diffs]
    assert np.all(np.ptp(blocks, axis=0).max(axis=1)[live] > 1e-3)
    axes = [i for i, k in enumerate(mc.kinds_of(*mc.case(name)[2:])[:run["table"][2]]) if k == mc.AXIS]
    assert axes and np.allclose(np.linalg.norm(blocks[:, axes], axis=2), 1.0, atol=1e-12)


@pytest.mark.parametrize("wrong", mc.WRONG)
def test_the_oracle_comparison_catches_a_wrong_interpreter(wrong):
    """Ball rates or free angular rates read in the world frame, the hinge anchor's lever arm dropped, the slide's w x (a d)
    dropped: each misses the velocities' bound by orders of magnitude on the cases built for it - and none moves a position."""
    caught = {}
    for name in mc.case_names():
        run = _run(name)
        program, n_rows, n_out, _, dofadr = run["table"]
        got = np.array([mc.interpret(program, n_rows, dofadr, n_out, q, qd, wrong=wrong) for q, qd in run["states"]])
        position, rate = _errors(run, got)
        assert position <= POSITION_BOUND
        if rate > RATE_BOUND:
            caught[name] = rate
    print(wrong, caught)
    must = {"ball_world": "random5", "free_world": "random17", "hinge_lever": "door", "slide_carry": "door"}[wrong]
    assert must in caught and caught[must] > 1e-3, caught


def test_reach_conditions():
    """What the cases must cover, asserted on the programs, the models and the states themselves."""
    seen = set()
    for name in mc.case_names():
        run = _run(name)
        raw, (program, n_rows, n_out, n_diff, dofadr) = run["raw"], run["table"]
        rows = program[:n_rows]
        closing = np.isin(rows[:, 0], mc.CLOSING)
        qd = np.array([s[1] for s in run["states"]])
        assert np.all(np.abs(qd) > 0)                               # every dof of every path has a non-zero rate
        turning = False                                             # an ancestor on this walk that rotates
        for k, row in enumerate(rows):
            kind = int(row[0])
            if closing[k]:
                if row[1] == 0:
                    turning = False
                continue
            seen.add(kind)
            assert 0 <= dofadr[k] < raw.nv
            if kind == mc.HINGE and turning and np.abs(row[13:16]).max() > 0:
                seen.add("anchored hinge under a rotating ancestor")
            if kind == mc.SLIDE and turning and abs(row[2]) + min(abs(q[int(row[1])] - row[2]) for q, _ in run["states"]) > 1e-3:
                seen.add("displaced slide under a rotating ancestor")
            if kind == mc.BALL and k > 0 and not closing[k - 1]:
                seen.add("ball below the root")
            if kind == mc.FREE and (k == 0 or closing[k - 1]):
                seen.add("free root")
            turning = turning or kind in (mc.HINGE, mc.BALL, mc.FREE)
        for _, body, _ in mc.resolved(raw, *mc.case(name)[2:])[0]:
            if any(raw.bodies[i].joint is None for i in pc.path(raw, body)):
                seen.add("folded welded body")
        if np.any(rows[closing][:, 1] == 1):
            seen.add("two outputs sharing one walk")
        slots = rows[closing][:, 2].astype(int)
        assert sorted(slots) == list(range(n_out))                  # every slot is named once
        if np.any(np.diff(slots) < 0):
            seen.add("slots out of program order")
        kinds = mc.kinds_of(*mc.case(name)[2:])
        if mc.VELOCITY in kinds[n_out:]:
            seen.add("difference of two velocities")
        seen |= {("closing", int(k)) for k in rows[closing][:, 0]}
    want = {mc.HINGE, mc.SLIDE, mc.BALL, mc.FREE, "anchored hinge under a rotating ancestor",
            "displaced slide under a rotating ancestor", "ball below the root", "free root", "folded welded body",
            "two outputs sharing one walk", "slots out of program order", "difference of two velocities",
            ("closing", mc.POINT), ("closing", mc.AXIS), ("closing", mc.VELOCITY), ("closing", mc.ANGULAR)}
    assert want <= seen, want - seen


# ---- the builder --------------------------------------------------------------------------------------------------------------
def test_a_point_and_its_velocity_share_one_walk():
    from mjmpc_amd.envs.cost_terms import CostTerms
    raw, kind, _, _ = mc.case("reacher")
    eng = pc.host_engine(raw, kind)
    deep = raw.bodies[pc.deepest(raw)].name
    nodes = sum(raw.bodies[b].joint is not None for b in pc.path(raw, pc.deepest(raw)))
    terms = CostTerms(eng).point("tip", body=deep, pos=(0.0, 0.0, 0.1)).velocity("tip_vel", "tip")
    program, n_rows, n_out, n_diff, dofadr = terms.points_table()
    assert (n_rows, n_out, n_diff) == (nodes + 2, 2, 0) and program.shape == (nodes + 2, 16)
    assert program[nodes:, 0].tolist() == [mc.POINT, mc.VELOCITY] and program[nodes:, 1].tolist() == [1.0, 0.0]
    assert program[nodes:, 2].tolist() == [0.0, 1.0]
    assert np.array_equal(program[nodes, 3:6], program[nodes + 1, 3:6])
    assert dofadr.tolist() == list(range(nodes)) + [0, 0]
    # the node rows are mjmpc_points' exactly
    plain = CostTerms(eng).point("tip", body=deep, pos=(0.0, 0.0, 0.1)).points_table()
    assert len(plain) == 4 and np.array_equal(plain[0][:nodes], program[:nodes])
    # a second body in between: the walks are grouped by body, so the slots leave program order
    mid = raw.bodies[pc.path(raw, pc.deepest(raw))[2]].name
    terms = CostTerms(eng).point("tip", body=deep).point("mid", body=mid).velocity("tip_vel", "tip")
    terms.angular_velocity("spin", body=mid).axis("mid_x", body=mid, axis=(3.0, 0.0, 0.0))
    program, n_rows, n_out, _, _ = terms.points_table()
    closing = program[:n_rows][np.isin(program[:n_rows, 0], mc.CLOSING)]
    assert closing[:, 2].tolist() == [0, 2, 1, 3, 4] and closing[:, 1].tolist() == [1, 0, 1, 1, 0]
    assert closing[4, 3:6].tolist() == [1.0, 0.0, 0.0]                                      # normalised by the host


def test_block_indices_and_rows():
    raw, eng, terms, outputs, differences = _terms("tray")
    d = eng.model.d_obs
    layout = terms.points_layout()
    assert list(layout) == [n for _, n, _ in outputs] + [n for n, _, _ in differences]
    assert [layout[k] for k in layout] == [slice(d + 3 * i, d + 3 * i + 3) for i in range(len(layout))]
    assert terms.n_extra == 3 * len(layout) and terms.needs_motion_entry
    terms.linear(obs="up0", index=2, weight=-2.0)
    terms.norm(obs="slip", weight=0.5)
    terms.square(obs="spin1", index=1, weight=0.1, terminal=True)
    terms.quadratic(parts=[dict(obs="glass_vel"), dict(obs="qvel", index=0)], matrix=np.eye(4))
    table = terms.table()
    want = [layout["up0"].start + 2] + list(range(layout["slip"].start, layout["slip"].stop)) + [layout["spin1"].start + 1] \
        + list(range(layout["glass_vel"].start, layout["glass_vel"].stop)) + [eng.obs_layout()["qvel"].start]
    assert table[:, 2].astype(int).tolist() == want
    with pytest.raises(ValueError, match="outside"):
        terms.square(obs=[d + terms.n_extra])


def test_refusals():
    from mjmpc_amd.envs.cost_terms import CostTerms
    from mjmpc_amd.models.half_cheetah import half_cheetah_raw
    raw, eng, terms, _, _ = _terms("tray")
    fresh = CostTerms(eng).point("glass", site="finger").point("tray", body="wrist")
    for bad in ((0.0, 0.0, 0.0), (0.0, float("nan"), 1.0), (float("inf"), 0.0, 0.0), (1.0, 0.0)):
        with pytest.raises(ValueError, match="axis"):
            fresh.axis("a", body="wrist", axis=bad)
    with pytest.raises(ValueError, match="axis="):
        fresh.axis("a", body="wrist")
    with pytest.raises(ValueError, match="unknown body"):
        fresh.axis("a", body="nobody", axis=(0, 0, 1))
    with pytest.raises(ValueError, match="unknown body"):
        fresh.angular_velocity("w", body="nobody")
    with pytest.raises(ValueError, match="unknown point"):
        fresh.velocity("v", "nothing")
    fresh.axis("up", body="wrist", axis=(0, 0, 1)).velocity("glass_vel", "glass").angular_velocity("spin", body="wrist")
    with pytest.raises(ValueError, match="unknown point"):
        fresh.velocity("v", "up")                                   # an axis is not a point
    for name in ("qpos", "glass", "up", "glass_vel", "spin"):       # an obs_layout block and every kind of output
        for build in (lambda n: fresh.axis(n, body="wrist", axis=(0, 0, 1)), lambda n: fresh.velocity(n, "glass"),
                      lambda n: fresh.angular_velocity(n, body="wrist")):
            with pytest.raises(ValueError, match="already"):
                build(name)
    # differences take two of one kind
    fresh.velocity("tray_vel", "tray").axis("side", body="wrist", axis=(1, 0, 0)).angular_velocity("spin2", body="elbow")
    for a, b in (("glass", "up"), ("glass", "glass_vel"), ("glass_vel", "spin"), ("up", "spin"), ("spin", "tray")):
        with pytest.raises(ValueError, match="different kinds"):
            fresh.difference("d", a, b)
    with pytest.raises(ValueError, match="unknown point"):
        fresh.difference("d", "glass_vel", "nothing")
    n = len(fresh.points_layout())
    for k in range(16 - n):
        fresh.axis("a%d" % k, body="wrist", axis=(0.1 * k, 1.0, 0.0))
    for build in (lambda: fresh.axis("x", body="wrist", axis=(0, 0, 1)), lambda: fresh.velocity("x", "glass"),
                  lambda: fresh.angular_velocity("x", body="wrist"), lambda: fresh.point("x", body="wrist")):
        with pytest.raises(ValueError, match="at most 16"):
            build()
    for k, (a, b) in enumerate([("glass_vel", "tray_vel"), ("up", "side"), ("spin", "spin2"), ("glass", "tray")] * 4):
        fresh.difference("d%d" % k, a, b)
    with pytest.raises(ValueError, match="at most 16 differences"):
        fresh.difference("d16", "up", "side")
    assert fresh.n_extra == 96
    for build in (lambda: terms.axis("late", body="wrist", axis=(0, 0, 1)), lambda: terms.velocity("late", "glass"),
                  lambda: terms.angular_velocity("late", body="wrist")):
        with pytest.raises(ValueError, match="before the differences"):
            build()
    for build in (lambda t: t.axis("a", body="wrist", axis=(0, 0, 1)), lambda t: t.velocity("v", "p"),
                  lambda t: t.angular_velocity("w", body="wrist")):
        with pytest.raises(ValueError, match="needs an engine"):
            build(CostTerms())
        compiled = pc.host_engine(raw, "tree")
        compiled.raw = None                                         # an engine made from a compiled model
        with pytest.raises(ValueError, match="built from a RawModel"):
            build(CostTerms(compiled))
        cheetah = pc.host_engine(half_cheetah_raw())                # TASK_FORWARD, obs_skip 1
        with pytest.raises(ValueError, match="leaves out"):
            build(CostTerms(cheetah))


def test_a_points_only_table_is_the_parents(monkeypatch):
    """The old tuple and the old program bit for bit, and the old entry: the new one is patched to raise."""
    from mjmpc_amd.envs import cost_terms as ct
    for name in pc.case_names():
        raw, kind, points, differences = pc.case(name)
        eng = pc.host_engine(raw, kind)
        terms = pc.add_points(ct.CostTerms(eng), points, differences)
        table = terms.points_table()
        pts, diffs = pc.resolved(raw, points, differences)
        program, n_rows = ct.points_program(raw, pts, diffs)
        assert len(table) == 4 and table[1:] == (n_rows, len(points), len(differences)) and not terms.needs_motion_entry
        assert np.array_equal(table[0], program) and np.all(program[:n_rows][program[:n_rows, 0] == 0][:, 1:3] == 0)

    # the launch: a host-only engine with a recording library in place of the device's
    class Lib:
        calls = []

        def mjmpc_points(self, *a):
            self.calls.append("mjmpc_points")
            return 0

        def mjmpc_points_motion(self, *a):
            raise AssertionError("a points-only table launched mjmpc_points_motion")

        def mjmpc_cost_terms(self, *a):
            self.calls.append("mjmpc_cost_terms")
            return 0

    import torch
    from mjmpc_amd.envs import _engine
    raw, kind, points, differences = pc.case("tray")
    eng = pc.host_engine(raw, kind)
    terms = pc.add_points(ct.CostTerms(eng), points, differences).abs(obs="glass")
    eng._lib, eng._code, eng.d_obs, eng.d_action = Lib(), 1, eng.model.d_obs, eng.model.nu
    eng._terms_dev, eng._cost_terms, eng._terms_read_actions = torch.zeros((3, 8), dtype=torch.float64), terms, False
    eng._points = (torch.from_numpy(terms.points_table()[0]),) + terms.points_table()[1:] + (terms.n_extra, None)
    monkeypatch.setattr(eng, "_buffer", lambda name, shape: torch.zeros(shape, dtype=torch.float64), raising=False)
    monkeypatch.setattr(eng, "_stream", lambda: None, raising=False)
    eng._launch_cost_terms(2, 3, torch.zeros((2, 3, eng.d_obs), dtype=torch.float64), None, torch.zeros((2, 3)), False)
    assert Lib.calls == ["mjmpc_points", "mjmpc_cost_terms"]


def test_programs_are_the_recorded_ones_byte_for_byte():
    """``points_program`` and ``motion_program`` - called directly and through ``CostTerms.points_table()`` - over every case of
    points_cases and motion_cases against tests/golden/points_programs.npz: every program, ``n_rows`` and, for motion, ``dofadr``,
    byte for byte and dtype for dtype.  The file was written by the two builders of commit 897adae - the last with a row loop of
    their own each - over the same cases (keys ``points/<case>/...`` and ``motion/<case>/...``)."""
    from mjmpc_amd.envs import cost_terms as ct
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "points_programs.npz")
    compared = 0

    def same(got, key):
        nonlocal compared
        want = golden[key]
        assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), key
        compared += 1

    with np.load(path) as golden:
        for name in pc.case_names():
            raw, kind, points, differences = pc.case(name)
            table = pc.add_points(ct.CostTerms(pc.host_engine(raw, kind)), points, differences).points_table()
            direct = ct.points_program(raw, *pc.resolved(raw, points, differences))
            for program, n_rows in (table[:2], direct):
                same(program, "points/%s/program" % name)
                assert n_rows == int(golden["points/%s/n_rows" % name]) and isinstance(n_rows, int)
            assert len(table) == 4 and len(direct) == 2
        for name in mc.case_names():
            raw, kind, outputs, differences = mc.case(name)
            table = mc.add_outputs(ct.CostTerms(pc.host_engine(raw, kind)), outputs, differences).points_table()
            direct = ct.motion_program(raw, *mc.resolved(raw, outputs, differences))
            for program, n_rows, dofadr in (table[:2] + table[4:], direct):
                same(program, "motion/%s/program" % name)
                same(dofadr, "motion/%s/dofadr" % name)
                assert n_rows == int(golden["motion/%s/n_rows" % name]) and isinstance(n_rows, int)
            assert len(table) == 5 and len(direct) == 3
        assert len(golden.files) == 5 * len(pc.case_names()) and compared == 6 * len(pc.case_names())


def test_config_blocks_parse_to_the_same_table_as_the_calls():
    from mjmpc_amd.envs.cost_terms import CostTerms, cost_terms_from_config
    raw, eng, _, _, _ = _terms("tray")
    block = dict(points=[dict(name="tray", body="wrist", pos=[0.0, 0.0, 0.02]), dict(name="glass", site="finger")],
                 axes=[dict(name="glass_up", body="wrist", axis=[0, 0, 2])],
                 velocities=[dict(name="glass_vel", point="glass"), dict(name="tray_vel", point="tray")],
                 angular_velocities=[dict(name="spin", body="wrist")],
                 differences=[dict(name="slip", a="glass_vel", b="tray_vel")],
                 terms=[dict(kind="linear", obs="glass_up", index=2, weight=[-1.0, -2.0, -4.0]),
                        dict(kind="norm", obs="slip", weight=0.5), dict(kind="square", obs="spin", weight=0.1)])
    each = cost_terms_from_config(block, eng, num_episodes=3)
    want = CostTerms(eng).point("tray", body="wrist", pos=(0.0, 0.0, 0.02)).point("glass", site="finger")
    want.axis("glass_up", body="wrist", axis=(0, 0, 1)).velocity("glass_vel", "glass").velocity("tray_vel", "tray")
    want.angular_velocity("spin", body="wrist").difference("slip", "glass_vel", "tray_vel")
    want.linear(obs="glass_up", index=2, weight=-2.0).norm(obs="slip", weight=0.5).square(obs="spin", weight=0.1)
    assert len(each) == 3 and np.array_equal(each[1].table(), want.table())
    for t in each:
        got, ref = t.points_table(), want.points_table()
        assert len(got) == 5 and got[1:4] == ref[1:4] and np.array_equal(got[0], ref[0]) and np.array_equal(got[4], ref[4])
        assert t.points_layout() == want.points_layout()
    for key, entry, match in (("axes", dict(name="a", body="wrist"), "an axis takes"),
                              ("velocities", dict(name="v", body="wrist"), "a velocity takes"),
                              ("angular_velocities", dict(name="w", point="glass"), "an angular velocity takes")):
        with pytest.raises(ValueError, match=match):
            cost_terms_from_config(dict(block, **{key: [entry]}), eng)


def test_batches_share_outputs_and_differences():
    from mjmpc_amd.control.batched import BatchedMPPI
    from mjmpc_amd.envs.cost_terms import CostTerms
    raw, eng, _, outputs, differences = _terms("tray")

    def table(e, outs=outputs):
        return mc.add_outputs(CostTerms(eng), outs, differences).linear(obs="up0", index=2, weight=-1.0 - e)
    tables = BatchedMPPI._resolve_cost_terms([table(e) for e in range(3)], eng, 3)[0]
    assert tables.shape[0] == 3 and tables[0, 0, 3] != tables[1, 0, 3]
    moved = [(b, n, dict(kw, axis=(0.0, 1.0, 0.0)) if n == "up1" else kw) for b, n, kw in outputs]
    with pytest.raises(ValueError, match="episode 1's points"):
        BatchedMPPI._resolve_cost_terms([table(0), table(1, moved), table(2)], eng, 3)
    plain = pc.add_points(CostTerms(eng), *pc.case("tray")[2:]).abs(obs="glass", index=0)
    with pytest.raises(ValueError, match="episode 1's (points|rows)"):           # (refused either way, naming the episode)
        BatchedMPPI._resolve_cost_terms([table(0), plain, table(2)], eng, 3)


def test_example_configs_resolve():
    import yaml
    from mjmpc_amd.envs.cost_terms import cost_terms_from_config
    raw, eng, _, _, _ = _terms("tray")
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples", "configs")
    with open(os.path.join(root, "tray_points_gpu.yml")) as f:
        base = cost_terms_from_config(yaml.safe_load(f)["cost_terms"], eng)
    with open(os.path.join(root, "tray_upright_gpu.yml")) as f:
        one = cost_terms_from_config(yaml.safe_load(f)["cost_terms"], eng)
    assert one.needs_motion_entry and len(one.points_table()) == 5 and one.points_table()[2:4] == (5, 2)
    assert np.array_equal(one.table()[:len(base.table())][:, [0, 1, 3, 4]], base.table()[:, [0, 1, 3, 4]])      # on top of the points config's terms
    assert list(one.points_layout())[:2] == list(base.points_layout())[:2]
    with open(os.path.join(root, "tray_upright_batch_gpu.yml")) as f:
        cfg = yaml.safe_load(f)
    each = cost_terms_from_config(cfg["cost_terms"], eng, num_episodes=cfg["n_episodes"])
    assert len(each) == cfg["n_episodes"] == 4
    upright = [i for i, r in enumerate(each[0].table()) if r[2] == each[0].points_layout()["glass_up"].start + 2]
    assert len(upright) == 1 and len({t.table()[upright[0], 3] for t in each}) == 4


# ---- the entry point ----------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_bound_and_exported():
    import batched_cases as bc
    from mjmpc_amd import _lib
    header = bc.check_entry_points(["mjmpc_points", "mjmpc_points_motion"], abi=4)
    assert len(_lib.SIGNATURES["mjmpc_points_motion"][1]) == 13 and len(_lib.SIGNATURES["mjmpc_points"][1]) == 11
    assert "const int32_t* d_dofadr" in header


def test_bad_arguments_are_codes_and_messages():
    from mjmpc_amd import _lib
    lib = _lib.load()
    p = 64          # (never dereferenced: every call below is refused before anything is launched)

    def call(dtype=_lib.F64, N=1, d_obs=6, nq=2, nv=2, obs=p, prog=p, dofadr=p, n_rows=1, n_out=1, n_diff=0, out=p):
        return lib.mjmpc_points_motion(dtype, N, d_obs, nq, nv, obs, prog, dofadr, n_rows, n_out, n_diff, out, None)
    for kw in (dict(obs=None), dict(prog=None), dict(out=None), dict(dofadr=None), dict(N=0), dict(d_obs=0), dict(nq=7), dict(nq=0),
               dict(nv=0), dict(nv=-1), dict(nv=5), dict(nq=6, nv=1), dict(n_out=0), dict(n_out=17), dict(n_diff=17),
               dict(n_diff=-1), dict(n_rows=0), dict(n_rows=545), dict(n_rows=2, n_out=3), dict(dtype=7), dict(d_obs=8000)):
        assert call(**kw) == -1, kw                 # MJMPC_E_BADARG
        assert lib.mjmpc_last_error().startswith(b"mjmpc_points_motion:"), (kw, lib.mjmpc_last_error())
    call(dofadr=None)
    assert b"d_dofadr" in lib.mjmpc_last_error()
    call(nv=5)
    assert b"nq + nv" in lib.mjmpc_last_error()
