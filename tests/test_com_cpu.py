"""CPU: centres of mass as cost-term observations - the tree program ``CostTerms.com`` / ``com_velocity`` build,
interpreted by tests/com_cases.py from the header's row format, against the C oracle; the builder, its refusals, the config
blocks and the C entry's argument checks.  Nothing here needs a GPU.

Positions are held to ``sum m_b x_b / sum m_b`` of the oracle at 1e-12 (the points' bound).  Velocities are held to the identity
``sum m_b v_b / M`` with ``v_b`` from ``motion_cases.interpret`` at 1e-12, and to the fourth-order central difference of the
oracle's centre of mass at RATE_BOUND: measured here over all cases the worst difference is 4.01e-11 (random35: a chain of 20
joints at rates of 2 rad/s; 5.1e-12 on the fixed models), the finite difference's own error; ten times that stands, under the cap of 1e-6."""
import os

import numpy as np
import pytest

import com_cases as cc
import motion_cases as mc
import points_cases as pc

N_STATES = 8
POSITION_BOUND = 1e-12
RATE_BOUND = 4.01e-10            # ten times the measured worst (the module's docstring); the cap is 1e-6


def _terms(name):
    from mjmpc_amd.envs.cost_terms import CostTerms
    raw, kind, outputs, differences = cc.case(name)
    eng = pc.host_engine(raw, kind)
    return raw, eng, cc.add_outputs(CostTerms(eng), outputs, differences), outputs, differences


_RUNS = {}


def _run(name):
    """The case's program interpreted at N_STATES random states, and the oracle's centres of mass and their rates there."""
    if name not in _RUNS:
        raw, eng, terms, outputs, differences = _terms(name)
        program, n_rows, n_out, n_diff, dofadr, n_levels = terms.points_table()
        rs = np.random.RandomState(11)
        states = [cc.random_state(raw, rs) for _ in range(N_STATES)]
        q, qd = np.array([s[0] for s in states]), np.array([s[1] for s in states])
        oracle = cc.Oracle(raw)
        names = [b.name for b in raw.bodies]
        part = names.index(outputs[2][2]["body"])
        want = dict(whole=np.array([oracle.com(None, x) for x in q]), part=np.array([oracle.com(part, x) for x in q]),
                    whole_vel=np.array([oracle.com_velocity(None, x, y) for x, y in zip(q, qd)]),
                    part_vel=np.array([oracle.com_velocity(part, x, y) for x, y in zip(q, qd)]))
        _RUNS[name] = dict(raw=raw, eng=eng, terms=terms, table=(program, n_rows, n_out, n_diff, dofadr, n_levels), q=q, qd=qd,
                           oracle=oracle, part=part, want=want, layout=terms.points_layout())
    return _RUNS[name]


def _got(run, wrong=None):
    program, n_rows, n_out, n_diff, dofadr, n_levels = run["table"]
    got = cc.interpret(program, n_rows, dofadr, n_out, n_levels, run["q"], run["qd"], wrong=wrong)
    d = run["eng"].model.d_obs
    return {k: got[:, s.start - d:s.stop - d] for k, s in run["layout"].items()}


def _errors(run, wrong=None):
    """-> (worst position error, worst rate error against the finite difference) over both centres of mass."""
    got, want = _got(run, wrong), run["want"]
    return (max(np.abs(got[k] - want[k]).max() for k in ("whole", "part")),
            max(np.abs(got[k] - want[k]).max() for k in ("whole_vel", "part_vel")))


@pytest.mark.parametrize("name", cc.case_names())
def test_interpreted_program_matches_the_oracle(name):
    from mjmpc_amd.envs import cost_terms as ct
    run = _run(name)
    raw, eng, oracle = run["raw"], run["eng"], run["oracle"]
    # the compiler's masses and inertial positions are the oracle's
    mass, ipos = ct.inertials(eng)
    assert mass.shape == oracle.mass.shape and np.abs(mass - oracle.mass).max() <= 1e-12 * max(1.0, oracle.mass.max())
    heavy = oracle.mass > 0
    assert np.abs(ipos[heavy] - oracle.ipos[heavy]).max() <= 1e-12
    pos_err, rate_err = _errors(run)
    print("%s: worst |com - oracle| %.3g, worst |com velocity - finite difference| %.3g" % (name, pos_err, rate_err))
    assert pos_err <= POSITION_BOUND
    assert rate_err <= RATE_BOUND <= 1e-6
    # the identity: the velocity is sum m_b v_b / M with v_b the velocity of the point at body b's inertial position
    got = _got(run)
    for key, body in (("whole_vel", None), ("part_vel", run["part"])):
        bodies = [b for b in cc.subtree(raw, body) if mass[b] > 0]
        total = 0.0
        for at in range(0, len(bodies), 16):         # (a table holds 16 outputs)
            chunk = bodies[at:at + 16]
            program, n_rows, dofadr = ct.motion_program(raw, [(mc.VELOCITY, b, ipos[b]) for b in chunk])
            v = mc.interpret(program, n_rows, dofadr, len(chunk), run["q"], run["qd"]).reshape(N_STATES, len(chunk), 3)
            total = total + np.einsum("b,nbc->nc", mass[chunk], v)
        assert np.abs(got[key] - total / mass[bodies].sum()).max() <= 1e-12, key
    # the ordinary point, its velocity and the differences beside them
    names = [b.name for b in raw.bodies]
    _, _, outputs, _ = cc.case(name)
    tip = (names.index(outputs[1][2]["body"]), np.asarray(outputs[1][2]["pos"], float))
    program, n_rows, dofadr = ct.motion_program(raw, [(mc.POINT,) + tip, (mc.VELOCITY,) + tip])
    plain = mc.interpret(program, n_rows, dofadr, 2, run["q"], run["qd"])
    assert np.array_equal(got["tip"], plain[:, :3]) and np.array_equal(got["tip_vel"], plain[:, 3:])
    assert np.array_equal(got["whole_from_tip"], got["whole"] - got["tip"])
    assert np.array_equal(got["part_from_whole_vel"], got["part_vel"] - got["whole_vel"])
    assert np.abs(got["part"] - got["whole"]).max() > 1e-3


@pytest.mark.parametrize("wrong", cc.WRONG)
def test_the_oracle_comparison_catches_a_wrong_interpreter(wrong):
    """Each deliberately wrong interpreter misses the bound on a case where the right one holds it."""
    name = {"restore": "hand24", "ipos": "cheetah", "lever": "cheetah", "shares": "swimmer"}[wrong]
    run = _run(name)
    pos_ok, rate_ok = _errors(run)
    assert pos_ok <= POSITION_BOUND and rate_ok <= RATE_BOUND
    pos_err, rate_err = _errors(run, wrong)
    if wrong == "lever":
        assert rate_err > 1e3 * RATE_BOUND and pos_err <= POSITION_BOUND        # (positions do not read the term)
    else:
        assert pos_err > 1e6 * POSITION_BOUND and rate_err > 1e3 * RATE_BOUND


def _levels_trace(program, n_rows):
    """-> (largest number of levels held at a time, whether a level is saved twice, whether a RESTORE names level -1)."""
    saves = [int(r[1]) for r in program[:n_rows] if int(r[0]) == cc.SAVE]
    restores = [int(r[1]) for r in program[:n_rows] if int(r[0]) == cc.RESTORE]
    return (max(saves) + 1 if saves else 0), len(saves) != len(set(saves)), -1 in restores


def test_the_cases_cover_what_they_must():
    from mjmpc_amd.envs import cost_terms as ct
    from mjmpc_amd.models.raw import JOINT_BALL, JOINT_FREE, JOINT_HINGE, JOINT_SLIDE
    nested = reused = world = welded = massless = below_root = False
    joint_kinds = set()
    for name in cc.case_names():
        run = _run(name)
        raw, eng = run["raw"], run["eng"]
        program, n_rows, n_out, n_diff, dofadr, n_levels = run["table"]
        held, twice, to_world = _levels_trace(program, n_rows)
        assert held == n_levels <= cc.MAX_LEVELS
        nested, reused, world = nested or n_levels >= 2, reused or twice, world or to_world
        mass, _ = ct.inertials(eng)
        inside = cc.subtree(raw, None)
        welded = welded or any(raw.bodies[b].joint is None and mass[b] > 0 and raw.bodies[b].parent >= 0 for b in inside)
        massless = massless or any(mass[b] == 0 for b in inside)
        below_root = below_root or raw.bodies[run["part"]].parent >= 0
        for body in (None, run["part"]):
            joint_kinds |= {raw.bodies[b].joint.type for b in cc.subtree(raw, body) if raw.bodies[b].joint is not None}
        # every jointed body of a subtree is visited once: as many node rows behind the path as it has joints
        assert len(dofadr) == n_rows and program.shape == (n_rows + n_diff, 16)
    assert nested and reused and world and welded and massless and below_root
    assert joint_kinds == {JOINT_HINGE, JOINT_SLIDE, JOINT_BALL, JOINT_FREE}


def test_row_counts_and_layout():
    """A subtree of ``n`` jointed bodies (``g`` of them massless groups) with ``b`` further children is
    ``path + 2 n - g + (saves + restores) + closing`` rows; every body is visited once."""
    from mjmpc_amd.envs import cost_terms as ct
    from mjmpc_amd.envs.cost_terms import CostTerms
    for name in cc.case_names():
        raw, eng, _, outputs, _ = _terms(name)
        mass, ipos = ct.inertials(eng)
        names = [b.name for b in raw.bodies]
        for body in (None, outputs[2][2]["body"]):
            terms = CostTerms(eng).com("c", body=body).com_velocity("cv", "c")
            program, n_rows, n_out, n_diff, dofadr, n_levels = terms.points_table()
            assert (n_out, n_diff) == (2, 0) and terms.n_extra == 6 and terms.needs_tree_entry
            root = -1 if body is None else names.index(body)
            inside = cc.subtree(raw, None if body is None else root)
            jointed = [b for b in inside if raw.bodies[b].joint is not None]
            path = 0 if body is None else sum(1 for b in pc.path(raw, root)[:-1] if raw.bodies[b].joint is not None)
            kinds = program[:n_rows, 0].astype(int)
            nodes = int(np.sum((kinds >= 1) & (kinds <= 4)))
            assert nodes == path + len(jointed)
            n_mass, n_save, n_restore = (int(np.sum(kinds == k)) for k in (cc.MASS, cc.SAVE, cc.RESTORE))
            assert n_rows == nodes + n_mass + n_save + n_restore + 2 and list(kinds[-2:]) == [cc.COM, cc.COM_VELOCITY]
            assert np.isclose(program[:n_rows][kinds == cc.MASS][:, 6].sum(), 1.0, rtol=0, atol=1e-15) and n_mass <= len(jointed) + 1
            assert np.all(program[:n_rows][kinds == cc.MASS][:, 6] > 0)
            # further children: one RESTORE each; a SAVE per branching node that is not the world
            assert program[n_rows - 2, 1] == 1 and program[n_rows - 2, 2] == 0 and tuple(program[n_rows - 1, 1:3]) == (0, 1)
            d = eng.model.d_obs
            assert terms.points_layout() == {"c": slice(d, d + 3), "cv": slice(d + 3, d + 6)}
    # hand24's hand: five fingers on the palm, which is welded to the wrist - one SAVE, four RESTOREs, one level
    raw, eng, _, _, _ = _terms("hand24")
    program, n_rows, _, _, _, n_levels = CostTerms(eng).com("hand", body="palm").points_table()
    kinds = program[:n_rows, 0].astype(int).tolist()
    assert n_levels == 1 and kinds.count(cc.SAVE) == 1 and kinds.count(cc.RESTORE) == 4
    assert kinds[:6] == [1, 1, 1, 1, cc.MASS, cc.SAVE] and n_rows == 4 + 1 + 1 + 4 + 2 * 20 + 1
    # the gripper's three root bodies: restores to the world frame, no level for them
    raw, eng, _, _, _ = _terms("gripper")
    program, n_rows, _, _, _, n_levels = CostTerms(eng).com("all").points_table()
    rows = program[:n_rows]
    assert [int(r[1]) for r in rows if int(r[0]) == cc.RESTORE][:2] == [-1, -1]


def test_refusals():
    from mjmpc_amd.envs.cost_terms import CostTerms
    raw, eng, terms, _, _ = _terms("tray")
    with pytest.raises(ValueError, match="unknown body"):
        CostTerms(eng).com("c", body="nobody")
    with pytest.raises(ValueError, match="exists already"):
        CostTerms(eng).com("c").com("c")
    with pytest.raises(ValueError, match="block of this engine's observation"):
        CostTerms(eng).com("qpos")
    with pytest.raises(ValueError, match="unknown centre of mass"):
        CostTerms(eng).point("p", body="wrist").com_velocity("v", "p")
    assert CostTerms(eng).com("c", body="wrist~0").points_table()[1] > 0       # (a massless body with a heavy child is fine)
    t = CostTerms(eng)
    for k in range(16):
        t.com("c%d" % k)
    with pytest.raises(ValueError, match="at most 16"):
        t.com("c16")
    with pytest.raises(ValueError, match="at most 16"):
        t.com_velocity("v", "c0")
    # differences: positions with positions, linear velocities with linear velocities
    t = CostTerms(eng).com("c").point("p", body="wrist").com_velocity("cv", "c").velocity("pv", "p").axis("a", body="wrist", axis=(0, 0, 1))
    t.angular_velocity("w", body="wrist")
    t.difference("d0", "c", "p").difference("d1", "p", "c").difference("d2", "cv", "pv").difference("d3", "cv", "cv")
    for a, b in (("c", "cv"), ("c", "pv"), ("cv", "p"), ("c", "a"), ("cv", "w"), ("a", "p")):
        with pytest.raises(ValueError, match="different kinds"):
            t.difference("bad", a, b)
    with pytest.raises(ValueError, match="before the differences"):
        t.com("late")
    # more saved frames than the kernel has
    deep = pc.host_engine(cc.comb(5))
    with pytest.raises(ValueError, match="5 saved frames"):
        CostTerms(deep).com("c")
    assert CostTerms(pc.host_engine(cc.comb(4))).com("c").points_table()[5] == 4
    # the conditions point() refuses
    with pytest.raises(ValueError, match="needs an engine"):
        CostTerms().com("c")
    from mjmpc_amd.models.half_cheetah import half_cheetah_raw
    with pytest.raises(ValueError, match="leaves out"):
        CostTerms(pc.host_engine(half_cheetah_raw())).com("c")
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    compiled = TreeRolloutEngine.host_only(raw)
    compiled.raw = None
    with pytest.raises(ValueError, match="built from a RawModel"):
        CostTerms(compiled).com("c")


def test_a_massless_subtree_is_refused():
    from mjmpc_amd.envs.cost_terms import CostTerms
    raw = cc.raw_model("comb2")
    assert not next(b for b in raw.bodies if b.name == "marker").geoms
    with pytest.raises(ValueError, match="weigh 0"):
        CostTerms(pc.host_engine(raw)).com("c", body="marker")


def test_body_mass_randomization_is_refused_in_both_orders(monkeypatch):
    from mjmpc_amd.control.batched import BatchedMPPI
    from mjmpc_amd.envs.cost_terms import CostTerms
    raw, eng, terms, _, _ = _terms("tray")
    terms.linear(obs="whole_vel", index=0, weight=-1.0)
    plain = CostTerms(eng).point("p", body="wrist").abs(obs="p")
    mass = {"body_mass": {"wrist": [0.1, 0.0]}}
    damping = {"dof_damping": {raw.joint_names[1]: [0.1, 0.0]}}
    # a host-only engine: the device calls are stubs
    import torch
    eng.num_shards, eng.device = 2, torch.device("cpu")
    eng.default_dyn_params, eng.randomized_dyn_params = [dict(), dict()], [dict(), dict()]
    monkeypatch.setattr(eng, "_fn", lambda name: (lambda *a: 0), raising=False)
    eng.d_action, eng._h = eng.model.nu, None
    eng.set_cost_terms(terms)
    with pytest.raises(ValueError, match="body_mass"):
        eng.randomize_dynamics(mass, 7)
    eng.randomize_dynamics(damping, 7)                  # anything else is allowed
    eng.set_cost_terms(plain)
    eng.randomize_dynamics(mass, 7)                     # ... and a table without a centre of mass takes body_mass
    with pytest.raises(ValueError, match="body_mass"):
        eng.set_cost_terms(terms)
    eng.set_cost_terms(plain)
    # a batch without a device: the same two orders
    b = BatchedMPPI.__new__(BatchedMPPI)
    b.engine, b.raw, b.model, b.num_episodes, b.num_particles = eng, raw, eng.model, 2, 8
    monkeypatch.setattr(b, "_tree_only", lambda what: None, raising=False)
    b._mass_randomized = {"body_mass": mass["body_mass"]}
    with pytest.raises(ValueError, match="body_mass"):
        b.set_cost_terms(terms)
    with pytest.raises(ValueError, match="body_mass"):
        b.set_cost_terms([terms, terms])
    b._mass_randomized, b._cost_terms_set = None, [terms, terms]
    with pytest.raises(ValueError, match="body_mass"):
        b.randomize_dynamics(mass, 7, 2)


def test_config_blocks_parse_to_the_same_table_as_the_calls():
    from mjmpc_amd.envs.cost_terms import CostTerms, cost_terms_from_config
    raw, eng, _, _, _ = _terms("tray")
    block = dict(points=[dict(name="tray", body="wrist", pos=[0.0, 0.0, 0.02])],
                 velocities=[dict(name="tray_vel", point="tray")],
                 coms=[dict(name="all"), dict(name="arm", body="shoulder")],
                 com_velocities=[dict(name="arm_vel", com="arm")],
                 differences=[dict(name="arm_from_tray", a="arm", b="tray"), dict(name="rel", a="arm_vel", b="tray_vel")],
                 terms=[dict(kind="linear", obs="arm_vel", index=0, weight=[-1.0, -2.0, -4.0]),
                        dict(kind="outside", obs="all", index=2, low=0.1, high=0.5, weight=3.0),
                        dict(kind="norm", obs="rel", weight=0.5)])
    each = cost_terms_from_config(block, eng, num_episodes=3)
    want = CostTerms(eng).point("tray", body="wrist", pos=(0.0, 0.0, 0.02)).velocity("tray_vel", "tray").com("all")
    want.com("arm", body="shoulder").com_velocity("arm_vel", "arm").difference("arm_from_tray", "arm", "tray")
    want.difference("rel", "arm_vel", "tray_vel").linear(obs="arm_vel", index=0, weight=-2.0)
    want.outside(obs="all", index=2, low=0.1, high=0.5, weight=3.0).norm(obs="rel", weight=0.5)
    assert len(each) == 3 and np.array_equal(each[1].table(), want.table())
    for t in each:
        got, ref = t.points_table(), want.points_table()
        assert len(got) == 6 and got[1:4] == ref[1:4] and got[5] == ref[5]
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[4], ref[4]) and t.points_layout() == want.points_layout()
    for key, entry, match in (("coms", dict(name="c", point="tray"), "a com takes"),
                              ("com_velocities", dict(name="v", body="wrist"), "a com velocity takes")):
        with pytest.raises(ValueError, match=match):
            cost_terms_from_config(dict(block, **{key: [entry]}), eng)


def test_example_configs_resolve():
    import yaml
    from mjmpc_amd.envs.cost_terms import cost_terms_from_config
    eng = cc.host_engine("cheetah")
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples", "configs")
    with open(os.path.join(root, "half_cheetah_com_gpu.yml")) as f:
        one = cost_terms_from_config(yaml.safe_load(f)["cost_terms"], eng)
    assert one.needs_tree_entry and one.keep_builtin and len(one.points_table()) == 6
    with open(os.path.join(root, "half_cheetah_com_batch_gpu.yml")) as f:
        cfg = yaml.safe_load(f)
    each = cost_terms_from_config(cfg["cost_terms"], eng, num_episodes=cfg["n_episodes"])
    assert len(each) == cfg["n_episodes"] and len({tuple(t.table()[:, 3]) for t in each}) == cfg["n_episodes"]
    assert all(np.array_equal(t.points_table()[0], one.points_table()[0]) for t in each)


def test_tables_without_a_centre_of_mass_are_the_parents(monkeypatch):
    """The old tuples and programs bit for bit, and the old entries: the new one is patched to raise."""
    from mjmpc_amd.envs import cost_terms as ct
    for name in pc.case_names():
        raw, kind, points, differences = pc.case(name)
        eng = pc.host_engine(raw, kind)
        table = pc.add_points(ct.CostTerms(eng), points, differences).points_table()
        program, n_rows = ct.points_program(raw, *pc.resolved(raw, points, differences))
        assert len(table) == 4 and table[1:] == (n_rows, len(points), len(differences)) and table[0].tobytes() == program.tobytes()
        raw, kind, outputs, differences = mc.case(name)
        terms = mc.add_outputs(ct.CostTerms(eng), outputs, differences)
        table = terms.points_table()
        program, n_rows, dofadr = ct.motion_program(raw, *mc.resolved(raw, outputs, differences))
        assert len(table) == 5 and table[1:4] == (n_rows, len(outputs), len(differences)) and not terms.needs_tree_entry
        assert table[0].tobytes() == program.tobytes() and table[4].tobytes() == dofadr.tobytes()
        # ... and the tree builder gives the same rows for such outputs: the row kinds mean what they meant
        again = ct.tree_program(raw, *mc.resolved(raw, outputs, differences))
        assert again[0].tobytes() == program.tobytes() and again[1] == n_rows and again[3] == 0
    assert ct.CostTerms(eng).abs(obs="qpos").points_table() is None

    class Lib:
        calls = []

        def mjmpc_points(self, *a):
            self.calls.append("mjmpc_points")
            return 0

        def mjmpc_points_motion(self, *a):
            self.calls.append("mjmpc_points_motion")
            return 0

        def mjmpc_points_tree(self, *a):
            if not self.allow:
                raise AssertionError("a table without a centre of mass launched mjmpc_points_tree")
            self.calls.append("mjmpc_points_tree:%d" % a[11])
            return 0

        def mjmpc_cost_terms(self, *a):
            self.calls.append("mjmpc_cost_terms")
            return 0

    import torch
    raw, kind, points, differences = pc.case("tray")
    eng = pc.host_engine(raw, kind)
    eng._lib, eng._code, eng.d_obs, eng.d_action, eng.device = Lib(), 1, eng.model.d_obs, eng.model.nu, torch.device("cpu")
    monkeypatch.setattr(eng, "_buffer", lambda name, shape: torch.zeros(shape, dtype=torch.float64), raising=False)
    monkeypatch.setattr(eng, "_stream", lambda: None, raising=False)

    def launch(terms, allow):
        Lib.calls, Lib.allow = [], allow
        eng.set_cost_terms(terms)
        eng._launch_cost_terms(2, 3, torch.zeros((2, 3, eng.d_obs), dtype=torch.float64), None, torch.zeros((2, 3)), False)
        return Lib.calls
    assert launch(pc.add_points(ct.CostTerms(eng), points, differences).abs(obs="glass"), False) == ["mjmpc_points", "mjmpc_cost_terms"]
    _, _, outputs, mdiff = mc.case("tray")
    assert launch(mc.add_outputs(ct.CostTerms(eng), outputs, mdiff).abs(obs="up0"), False) == ["mjmpc_points_motion", "mjmpc_cost_terms"]
    _, _, outputs, cdiff = cc.case("tray")
    assert launch(cc.add_outputs(ct.CostTerms(eng), outputs, cdiff).abs(obs="whole"), True) == ["mjmpc_points_tree:0", "mjmpc_cost_terms"]
    assert launch(ct.CostTerms(eng).abs(obs="qpos"), False) == ["mjmpc_cost_terms"]


def test_batches_share_centres_of_mass():
    from mjmpc_amd.control.batched import BatchedMPPI
    from mjmpc_amd.envs.cost_terms import CostTerms
    raw, eng, _, outputs, differences = _terms("tray")

    def table(e, outs=outputs):
        return cc.add_outputs(CostTerms(eng), outs, differences).linear(obs="whole_vel", index=0, weight=-1.0 - e)
    tables = BatchedMPPI._resolve_cost_terms([table(e) for e in range(3)], eng, 3)[0]
    assert tables.shape[0] == 3 and tables[0, 0, 3] != tables[1, 0, 3]
    moved = [(b, n, dict(body="wrist") if n == "part" else kw) for b, n, kw in outputs]
    assert not np.array_equal(table(0, moved).points_table()[0], table(0).points_table()[0])
    with pytest.raises(ValueError, match="episode 1's points"):
        BatchedMPPI._resolve_cost_terms([table(0), table(1, moved), table(2)], eng, 3)


# ---- the entry point ----------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_bound_and_exported():
    import batched_cases as bc
    from mjmpc_amd import _lib
    header = bc.check_entry_points(["mjmpc_points", "mjmpc_points_motion", "mjmpc_points_tree"], abi=4)
    assert len(_lib.SIGNATURES["mjmpc_points_tree"][1]) == len(_lib.SIGNATURES["mjmpc_points_motion"][1]) + 1 == 14
    assert "int n_levels" in header and "9 MASS" in header and "13 COM_VELOCITY" in header


def test_bad_arguments_are_codes_and_messages():
    from mjmpc_amd import _lib
    lib = _lib.load()
    p = 64          # (never dereferenced: every call below is refused before anything is launched)

    def call(dtype=_lib.F64, N=1, d_obs=6, nq=2, nv=2, obs=p, prog=p, dofadr=p, n_rows=1, n_out=1, n_diff=0, n_levels=0, out=p):
        return lib.mjmpc_points_tree(dtype, N, d_obs, nq, nv, obs, prog, dofadr, n_rows, n_out, n_diff, n_levels, out, None)
    # (d_obs 7650: such a row of doubles fits the tile with its one output, not with four levels' 416 bytes more)
    for kw in (dict(obs=None), dict(prog=None), dict(out=None), dict(dofadr=None), dict(N=0), dict(d_obs=0), dict(nq=7), dict(nq=0),
               dict(nv=0), dict(nv=-1), dict(nv=5), dict(nq=6, nv=1), dict(n_out=0), dict(n_out=17), dict(n_diff=17),
               dict(n_diff=-1), dict(n_rows=0), dict(n_rows=545), dict(n_rows=2, n_out=3), dict(dtype=7), dict(d_obs=8000),
               dict(n_levels=-1), dict(n_levels=5), dict(d_obs=7650, n_levels=4)):
        assert call(**kw) == -1, kw                 # MJMPC_E_BADARG
        assert lib.mjmpc_last_error().startswith(b"mjmpc_points_tree:"), (kw, lib.mjmpc_last_error())
    call(n_levels=5)
    assert b"n_levels" in lib.mjmpc_last_error()
    call(d_obs=7650, n_levels=4)
    assert b"saved frames" in lib.mjmpc_last_error()


def test_synthetic_programs_cover_the_tiles_and_the_guards():
    """What tests/test_com_gpu.py launches at the C entry: every ``n_levels``, tiles that the saved frames change, the edges of
    N, levels outside the range, a level never saved, a share of 0, two centre-of-mass walks - and a reference that notices each
    of the wrong interpreters."""
    import points_tile_cases as ptc
    cases = cc.synthetic_cases()
    for dtype in ("f64", "f32"):
        mine = [c for c in cases if c.dtype == dtype]
        assert {c.n_levels for c in mine} == set(range(cc.MAX_LEVELS + 1)) and len({c.tile for c in mine}) >= 3
        by_width = {}
        for c in mine:
            if not c.tags and c.N == ptc._ragged(c.tile):
                by_width.setdefault(c.d_obs, {})[c.n_levels] = c.tile
        assert any(t[0] > t[4] for t in by_width.values())                   # the levels cost rows of the tile
        assert {c.N - c.tile for c in mine if c.N <= c.tile + 1} >= {0, 1} and any(c.N == 1 for c in mine)
        assert any("wild" in c.tags for c in mine) and any("never saved" in c.tags for c in mine)
    for c in cases:
        assert c.tile == cc.tree_tile_rows(c.dtype, c.d_obs, c.n_out, c.n_levels)
        assert cc.tree_lds_bytes(c.dtype, c.d_obs, c.n_out, c.n_levels, c.tile) <= ptc.LDS_BYTES
        assert c.tile == 256 or cc.tree_lds_bytes(c.dtype, c.d_obs, c.n_out, c.n_levels, 2 * c.tile) > ptc.LDS_BYTES
        kinds = c.program[:c.n_rows, 0].astype(int)
        levels = c.program[:c.n_rows, 1].astype(int)[(kinds == cc.SAVE) | (kinds == cc.RESTORE)]
        if "wild" in c.tags:
            assert levels.max() >= c.n_levels and levels.min() < -1
        else:
            assert levels.size == 0 or (-1 <= levels.min() and levels.max() < c.n_levels)
    c = cc.synthetic_case("tree-f64-l3-d0")
    want80, interp64, b = cc.synthetic_reference(c.name)
    assert ptc.excess_f64(interp64, want80, b)[0] <= 0.0
    for wrong in cc.WRONG:
        assert ptc.excess_f64(cc.synthetic_interpret(c, np.float64, wrong), want80, b)[0] > 1e-6, wrong
    never = cc.synthetic_case("tree-f64-never-saved")
    saves = never.program[:never.n_rows][never.program[:never.n_rows, 0] == cc.SAVE][:, 1].astype(int).tolist()
    assert never.n_levels - 1 not in saves and never.n_levels - 1 in never.program[:never.n_rows, 1].astype(int).tolist()

