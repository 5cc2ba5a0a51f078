"""CPU: orientation errors as cost-term observations - the program ``CostTerms.orientation`` builds, interpreted by
tests/orient_cases.py from the header's row format, against the C oracle; the builder, its refusals, the config blocks and the C
entry's argument checks.  Nothing here needs a GPU.

The oracle's rotation vector comes from rotation matrices built of world points (orient_cases.Oracle), the interpreter's from the
header's log map over quaternions.  Measured here over all cases and their 8 states the worst difference is 7.55e-15 (random17: a
path of 15 joints; 8.9e-16 on the fixed models); ten times that stands, under the cap of 1e-9.

Near ``theta = pi`` the sign of ``r`` flips and the matrix route is ill-conditioned, so a draw with an angle above ``pi - 0.05``
for any orientation of its case is drawn again, and at most 1 draw in 20 of a case may be: with 8 states that is none.  Measured
over seeds 1 .. 399 a draw of these cases lands in the band with a frequency of 3.8 % (a uniform rotation does so with probability
``2 * 0.05 / pi`` = 3.2 % per orientation: the density of its angle is ``(1 - cos theta) / pi``), so the states' seed is one under
which no case draws again - STATE_SEED, the first of 31 .. 399 - and the test asserts the cap."""
import os

import numpy as np
import pytest

import com_cases as cc
import motion_cases as mc
import orient_cases as oc
import points_cases as pc

N_STATES = 8
STATE_SEED = 301
ORIENT_BOUND = oc.ORIENT_BOUND


def _terms(name):
    from mjmpc_amd.envs.cost_terms import CostTerms
    raw, kind, outputs, differences = oc.case(name)
    eng = pc.host_engine(raw, kind)
    return raw, eng, oc.add_outputs(CostTerms(eng), outputs, differences), outputs, differences


_RUNS = {}


def _run(name):
    """The case's program, N_STATES random states outside the band and the oracle's orientation errors there."""
    if name not in _RUNS:
        raw, eng, terms, outputs, differences = _terms(name)
        table = terms.points_table()
        specs = oc.resolved(raw, outputs)
        oracle = oc.Oracle(raw)
        q, qd, drawn = oc.draw_states(raw, oracle, specs, N_STATES, STATE_SEED)
        want = {k: np.array([oracle.error(s, x) for x in q]) for k, s in specs.items()}
        _RUNS[name] = dict(raw=raw, eng=eng, terms=terms, table=table, q=q, qd=qd, drawn=drawn, want=want, specs=specs,
                           layout=terms.points_layout(), outputs=outputs, differences=differences)
    return _RUNS[name]


def _got(run, wrong=None):
    program, n_rows, n_out, n_diff, dofadr, n_levels = run["table"][:6]
    got = oc.interpret(program, n_rows, dofadr, n_out, n_levels, run["q"], run["qd"], wrong=wrong)
    d = run["eng"].model.d_obs
    return {k: got[:, s.start - d:s.stop - d] for k, s in run["layout"].items()}


def _error(run, wrong=None):
    got = _got(run, wrong)
    return max(np.abs(got[k] - w).max() for k, w in run["want"].items())


@pytest.mark.parametrize("name", oc.case_names())
def test_interpreted_program_matches_the_oracle(name):
    from mjmpc_amd.envs import cost_terms as ct
    run = _run(name)
    raw = run["raw"]
    redrawn = run["drawn"] - N_STATES
    assert 20 * redrawn <= run["drawn"], "%s: %d of %d draws stood in the band below pi" % (name, redrawn, run["drawn"])
    err = _error(run)
    angles = np.concatenate([np.linalg.norm(w, axis=1) for w in run["want"].values()])
    print("%s: worst |orientation - oracle| %.3g, angles %.3f .. %.3f" % (name, err, angles.min(), angles.max()))
    assert err <= ORIENT_BOUND <= 1e-9
    assert angles.max() <= np.pi - oc.BAND and angles.max() > 1.0 and set(run["want"]) == {"to_ancestor", "absolute", "across"}
    # the other outputs of the table: the same definitions through the older builders and interpreters, to the bit
    got = _got(run)
    names = [b.name for b in raw.bodies]
    tip_kw = run["outputs"][0][2]
    tip = (names.index(tip_kw["body"]), np.asarray(tip_kw["pos"], float))
    program, n_rows, dofadr = ct.motion_program(raw, [(mc.POINT,) + tip, (mc.VELOCITY,) + tip, (mc.ANGULAR, tip[0], np.zeros(3))])
    plain = mc.interpret(program, n_rows, dofadr, 3, run["q"], run["qd"])
    assert np.array_equal(got["tip"], plain[:, :3]) and np.array_equal(got["tip_vel"], plain[:, 3:6])
    assert np.array_equal(got["spin"], plain[:, 6:9])
    if name == "cheetah":
        program, n_rows, dofadr, n_levels = ct.tree_program(raw, [(cc.COM, -1, None), (cc.COM_VELOCITY, 0, None)], (),
                                                            *ct.inertials(run["eng"]))
        com = cc.interpret(program, n_rows, dofadr, 2, n_levels, run["q"], run["qd"])
        assert run["table"][5] == n_levels > 0
        assert np.array_equal(got["whole"], com[:, :3]) and np.array_equal(got["whole_vel"], com[:, 3:])
        assert np.array_equal(got["tip_from_whole"], got["tip"] - got["whole"])


@pytest.mark.parametrize("wrong", oc.WRONG)
def test_the_oracle_comparison_catches_a_wrong_interpreter(wrong):
    """Each deliberately wrong interpreter misses the bound on every fixed model, where the right one holds it."""
    for name in ("reacher", "tray", "hand24", "pen_hand", "gripper", "cheetah"):
        run = _run(name)
        assert _error(run) <= ORIENT_BOUND
        assert _error(run, wrong) > 1e6 * ORIENT_BOUND, (name, wrong)


def test_the_cases_cover_what_they_must():
    from mjmpc_amd.models.raw import JOINT_BALL, JOINT_FREE, JOINT_HINGE, JOINT_SLIDE
    joint_kinds, branches, levels, flipped = set(), 0, False, False
    for name in oc.case_names():
        run = _run(name)
        raw = run["raw"]
        program, n_rows, n_out, n_diff, dofadr, n_levels, orient = run["table"]
        assert orient is True and run["terms"].needs_orient_entry and len(dofadr) == n_rows
        rows = program[:n_rows]
        closing = [int(r[2]) for r in rows if int(r[0]) in oc.CLOSING]
        assert sorted(closing) == list(range(n_out)) and closing != sorted(closing)        # the slots are out of program order
        specs = run["specs"]
        for body, o, g, other in specs.values():
            joint_kinds |= {raw.bodies[b].joint.type for b in pc.path(raw, body) if raw.bodies[b].joint is not None}
        a, b = specs["across"][0], specs["across"][3]
        branches += a not in pc.path(raw, b) and b not in pc.path(raw, a)
        assert specs["to_ancestor"][3] in pc.path(raw, specs["to_ancestor"][0])[:-1] or len(pc.path(raw, specs["to_ancestor"][0])) == 1
        assert specs["absolute"][2][0] < 0 and abs(specs["absolute"][1][0]) < 0.99            # a target with w < 0, a quat
        # the absolute orientation shares the point's walk: one walk holds POINT, ORIENTATION, VELOCITY and ANGULAR rows
        kinds = rows[:, 0].astype(int).tolist()
        at = kinds.index(oc.POINT)
        assert kinds[at:at + 4] == [oc.POINT, oc.ORIENTATION, oc.VELOCITY, oc.ANGULAR] and list(rows[at:at + 4, 1]) == [1, 1, 1, 0]
        levels = levels or n_levels > 0
        walk = oc.orientation_walk(program, n_rows, n_levels, run["q"])
        flipped = flipped or any(np.any(w < 0) for _, w in walk.values())
    assert joint_kinds == {JOINT_HINGE, JOINT_SLIDE, JOINT_BALL, JOINT_FREE}
    assert branches >= 5 and levels and flipped


def test_row_counts_and_layout():
    """An absolute orientation is its body's path and one row; a relative one both paths and two rows."""
    from mjmpc_amd.envs import cost_terms as ct
    from mjmpc_amd.envs.cost_terms import CostTerms
    for name in oc.case_names():
        raw, eng, _, outputs, _ = _terms(name)
        names = [b.name for b in raw.bodies]
        d = eng.model.d_obs

        def nodes(body):
            return sum(1 for b in pc.path(raw, names.index(body)) if raw.bodies[b].joint is not None)
        for _, _, kw in [o for o in outputs if o[0] == "orientation"]:
            terms = CostTerms(eng).orientation("r", **kw)
            program, n_rows, n_out, n_diff, dofadr, n_levels, orient = terms.points_table()
            assert (n_out, n_diff, n_levels, orient) == (1, 0, 0, True) and terms.n_extra == 3
            assert terms.needs_orient_entry and terms.needs_motion_entry and not terms.needs_tree_entry
            assert terms.points_layout() == {"r": slice(d, d + 3)} and program.shape == (n_rows, 16) and len(dofadr) == n_rows
            kinds = program[:, 0].astype(int).tolist()
            if "relative_to" in kw:
                first = nodes(kw["relative_to"])
                assert n_rows == first + nodes(kw["body"]) + 2
                assert kinds[first] == oc.HOLD and not np.any(program[first, 1:]) and kinds.count(oc.HOLD) == 1
                assert program[-1, 11] == 1
            else:
                assert n_rows == nodes(kw["body"]) + 1 and oc.HOLD not in kinds and program[-1, 11] == 0
            assert kinds[-1] == oc.ORIENTATION and tuple(program[-1, 1:3]) == (0, 0) and not np.any(program[-1, 12:])
            assert abs(np.linalg.norm(program[-1, 3:7]) - 1) < 1e-15 and abs(np.linalg.norm(program[-1, 7:11]) - 1) < 1e-15
    # the defaults are the identity, and a quaternion is normalised with its sign
    raw, eng, _, _, _ = _terms("tray")
    row = CostTerms(eng).orientation("r", body="glass").points_table()[0][-1]
    assert list(row[3:12]) == [1, 0, 0, 0, 1, 0, 0, 0, 0]
    row = CostTerms(eng).orientation("r", body="glass", quat=(0, -2, 0, 0), target=(-3, 0, 0, 4)).points_table()[0][-1]
    assert np.allclose(row[3:11], [0, -1, 0, 0, -0.6, 0, 0, 0.8], rtol=0, atol=1e-16)
    # orientations beside points stay in definition order, differences behind them
    t = CostTerms(eng).point("p", body="wrist").orientation("r", body="glass").point("g", body="glass").difference("d", "g", "p")
    d = eng.model.d_obs
    assert t.points_layout() == {"p": slice(d, d + 3), "r": slice(d + 3, d + 6), "g": slice(d + 6, d + 9), "d": slice(d + 9, d + 12)}
    assert t.n_extra == 12 and len(t.points_table()) == 7


def test_refusals():
    from mjmpc_amd.envs.cost_terms import CostTerms
    raw, eng, _, _, _ = _terms("tray")
    with pytest.raises(ValueError, match="unknown body"):
        CostTerms(eng).orientation("r", body="nobody")
    with pytest.raises(ValueError, match="unknown body"):
        CostTerms(eng).orientation("r", body="glass", relative_to="nobody")
    with pytest.raises(ValueError, match="takes body="):
        CostTerms(eng).orientation("r")
    with pytest.raises(ValueError, match="exists already"):
        CostTerms(eng).orientation("r", body="glass").orientation("r", body="wrist")
    with pytest.raises(ValueError, match="exists already"):
        CostTerms(eng).point("r", body="glass").orientation("r", body="wrist")
    with pytest.raises(ValueError, match="block of this engine's observation"):
        CostTerms(eng).orientation("qpos", body="glass")
    with pytest.raises(ValueError, match="not both"):
        CostTerms(eng).orientation("r", body="glass", target=(1, 0, 0, 0), relative_to="wrist")
    with pytest.raises(ValueError, match="goes with relative_to"):
        CostTerms(eng).orientation("r", body="glass", relative_quat=(1, 0, 0, 0))
    for key in ("quat", "target"):
        for bad, match in (((0, 0, 0, 0), "must not be zero"), ((1, 0, float("nan"), 0), "must be finite"),
                           ((1, float("inf"), 0, 0), "must be finite"), ((1, 0, 0), "four numbers")):
            with pytest.raises(ValueError, match=match):
                CostTerms(eng).orientation("r", body="glass", **{key: bad})
    with pytest.raises(ValueError, match="must not be zero"):
        CostTerms(eng).orientation("r", body="glass", relative_to="wrist", relative_quat=(0, 0, 0, 0))
    t = CostTerms(eng)
    for k in range(16):
        t.orientation("r%d" % k, body="glass")
    with pytest.raises(ValueError, match="at most 16"):
        t.orientation("r16", body="glass")
    # differences: subtracting rotation vectors is not a rotation
    t = CostTerms(eng).orientation("r", body="glass").orientation("s", body="wrist").point("p", body="wrist")
    t.angular_velocity("w", body="glass")
    for a, b in (("r", "s"), ("r", "p"), ("p", "r"), ("w", "r"), ("r", "r")):
        with pytest.raises(ValueError, match="relative_to"):
            t.difference("bad", a, b)
    t.difference("fine", "p", "p")
    with pytest.raises(ValueError, match="before the differences"):
        t.orientation("late", body="glass")
    # the conditions point() refuses
    with pytest.raises(ValueError, match="needs an engine"):
        CostTerms().orientation("r", body="glass")
    from mjmpc_amd.models.half_cheetah import half_cheetah_raw
    with pytest.raises(ValueError, match="leaves out"):
        CostTerms(pc.host_engine(half_cheetah_raw())).orientation("r", body="torso")
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    compiled = TreeRolloutEngine.host_only(raw)
    compiled.raw = None
    with pytest.raises(ValueError, match="built from a RawModel"):
        CostTerms(compiled).orientation("r", body="glass")


def test_body_mass_randomization_is_not_refused():
    """Nothing in an orientation depends on a mass."""
    from mjmpc_amd.envs.cost_terms import CostTerms, refuse_mass_randomization
    raw, eng, _, _, _ = _terms("tray")
    terms = CostTerms(eng).orientation("r", body="glass", relative_to="wrist").norm(obs="r")
    refuse_mass_randomization(terms, {"body_mass": {"wrist": [0.1, 0.0]}})
    with pytest.raises(ValueError, match="body_mass"):
        refuse_mass_randomization(CostTerms(eng).orientation("r", body="glass").com("c").abs(obs="c"),
                                  {"body_mass": {"wrist": [0.1, 0.0]}})


def test_config_blocks_parse_to_the_same_table_as_the_calls():
    from mjmpc_amd.envs.cost_terms import CostTerms, cost_terms_from_config
    raw, eng, _, _, _ = _terms("tray")
    block = dict(points=[dict(name="tray", body="wrist", pos=[0.0, 0.0, 0.02])],
                 angular_velocities=[dict(name="spin", body="glass")],
                 coms=[dict(name="all")],
                 orientations=[dict(name="level", body="glass", relative_to="wrist", relative_quat=[1.0, 0.0, 0.0, 0.1]),
                               dict(name="pose", body="glass", quat=[0.0, 1.0, 0.0, 0.0], target=[0.5, 0.5, -0.5, 0.5])],
                 differences=[dict(name="all_from_tray", a="all", b="tray")],
                 terms=[dict(kind="norm", obs="level", weight=[1.0, 2.0, 4.0]),
                        dict(kind="outside", obs="pose", index=2, low=-0.1, high=0.1, weight=3.0),
                        dict(kind="quadratic", parts=[dict(obs="level"), dict(obs="spin")], matrix=[1, 1, 1, 0.1, 0.1, 0.1]),
                        dict(kind="square", obs="pose", weight=0.5, terminal=True)])
    each = cost_terms_from_config(block, eng, num_episodes=3)
    want = CostTerms(eng).point("tray", body="wrist", pos=(0.0, 0.0, 0.02)).angular_velocity("spin", body="glass").com("all")
    want.orientation("level", body="glass", relative_to="wrist", relative_quat=(1.0, 0.0, 0.0, 0.1))
    want.orientation("pose", body="glass", quat=(0.0, 1.0, 0.0, 0.0), target=(0.5, 0.5, -0.5, 0.5))
    want.difference("all_from_tray", "all", "tray").norm(obs="level", weight=2.0)
    want.outside(obs="pose", index=2, low=-0.1, high=0.1, weight=3.0)
    want.quadratic(parts=[dict(obs="level"), dict(obs="spin")], matrix=[1, 1, 1, 0.1, 0.1, 0.1])
    want.square(obs="pose", weight=0.5, terminal=True)
    assert len(each) == 3 and np.array_equal(each[1].table(), want.table())
    for t in each:
        got, ref = t.points_table(), want.points_table()
        assert len(got) == 7 and got[1:4] == ref[1:4] and got[5:] == ref[5:]
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[4], ref[4]) and t.points_layout() == want.points_layout()
    for entry, match in ((dict(name="r", body="glass", axis=[0, 0, 1]), "an orientation takes"),
                         (dict(name="r"), "an orientation takes"), (dict(body="glass"), "an orientation takes")):
        with pytest.raises(ValueError, match=match):
            cost_terms_from_config(dict(block, orientations=[entry]), eng)
    with pytest.raises(ValueError, match="expected a mapping"):
        cost_terms_from_config(dict(block, orientation=[]), eng)


def test_example_configs_resolve():
    import yaml
    from mjmpc_amd.envs.cost_terms import cost_terms_from_config
    eng = oc.host_engine("tray")
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples", "configs")
    with open(os.path.join(root, "tray_level_gpu.yml")) as f:
        one = cost_terms_from_config(yaml.safe_load(f)["cost_terms"], eng)
    assert one.needs_orient_entry and one.keep_builtin and len(one.points_table()) == 7
    rows = one.points_table()[0]
    assert rows[:, 0].astype(int).tolist().count(oc.HOLD) == 1 and "glass_on_tray" in one.points_layout()
    with open(os.path.join(root, "tray_points_gpu.yml")) as f:
        base = cost_terms_from_config(yaml.safe_load(f)["cost_terms"], eng)
    assert np.array_equal(one.table()[:len(base.table()), :2], base.table()[:, :2]) and len(one.table()) == len(base.table()) + 3
    with open(os.path.join(root, "tray_level_batch_gpu.yml")) as f:
        cfg = yaml.safe_load(f)
    each = cost_terms_from_config(cfg["cost_terms"], eng, num_episodes=cfg["n_episodes"])
    assert len(each) == cfg["n_episodes"] and len({tuple(t.table()[:, 3]) for t in each}) == cfg["n_episodes"]
    assert all(np.array_equal(t.points_table()[0], one.points_table()[0]) for t in each)


def test_tables_without_an_orientation_are_the_parents(monkeypatch):
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
        assert len(table) == 5 and table[1:4] == (n_rows, len(outputs), len(differences)) and not terms.needs_orient_entry
        assert table[0].tobytes() == program.tobytes() and table[4].tobytes() == dofadr.tobytes()
    golden = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "orient_parent_tables.npz"))
    for name in cc.case_names():
        raw, kind, outputs, differences = cc.case(name)
        terms = cc.add_outputs(ct.CostTerms(pc.host_engine(raw, kind)), outputs, differences)
        table = terms.points_table()
        assert len(table) == 6 and not terms.needs_orient_entry and terms.needs_tree_entry
        assert table[0].tobytes() == golden[name + "/program"].tobytes() and table[4].tobytes() == golden[name + "/dofadr"].tobytes()
        assert table[1:4] + table[5:] == tuple(int(x) for x in golden[name + "/counts"])

    class Lib:
        calls = []

        def mjmpc_points(self, *a):
            self.calls.append("mjmpc_points")
            return 0

        def mjmpc_points_motion(self, *a):
            self.calls.append("mjmpc_points_motion")
            return 0

        def mjmpc_points_tree(self, *a):
            self.calls.append("mjmpc_points_tree:%d" % a[11])
            return 0

        def mjmpc_points_orient(self, *a):
            if not self.allow:
                raise AssertionError("a table without an orientation launched mjmpc_points_orient")
            self.calls.append("mjmpc_points_orient:%d" % a[11])
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
    assert launch(cc.add_outputs(ct.CostTerms(eng), outputs, cdiff).abs(obs="whole"), False) == ["mjmpc_points_tree:0", "mjmpc_cost_terms"]
    assert launch(ct.CostTerms(eng).abs(obs="qpos"), False) == ["mjmpc_cost_terms"]
    _, _, outputs, odiff = oc.case("tray")
    assert launch(oc.add_outputs(ct.CostTerms(eng), outputs, odiff).norm(obs="across"), True) == ["mjmpc_points_orient:0",
                                                                                                 "mjmpc_cost_terms"]
    assert eng._points_orient
    assert launch(ct.CostTerms(eng).abs(obs="qpos"), False) == ["mjmpc_cost_terms"] and not eng._points_orient
    # a table with a centre of mass beside an orientation: the whole program through the new entry, with its levels
    raw, kind, outputs, odiff = oc.case("cheetah")
    terms = oc.add_outputs(ct.CostTerms(pc.host_engine(raw, kind)), outputs, odiff)
    assert terms.points_table()[5] > 0 and terms.needs_tree_entry and terms.needs_orient_entry


def test_batches_share_orientations():
    from mjmpc_amd.control.batched import BatchedMPPI
    from mjmpc_amd.envs.cost_terms import CostTerms
    raw, eng, _, outputs, differences = _terms("tray")

    def table(e, outs=outputs):
        return oc.add_outputs(CostTerms(eng), outs, differences).norm(obs="across", weight=1.0 + e)
    tables = BatchedMPPI._resolve_cost_terms([table(e) for e in range(3)], eng, 3)[0]
    assert tables.shape[0] == 3 and tables[0, 0, 3] != tables[1, 0, 3]
    moved = [(b, n, dict(kw, quat=(0.0, 0.0, 1.0, 0.0)) if n == "absolute" else kw) for b, n, kw in outputs]
    assert not np.array_equal(table(0, moved).points_table()[0], table(0).points_table()[0])
    with pytest.raises(ValueError, match="episode 1's points"):
        BatchedMPPI._resolve_cost_terms([table(0), table(1, moved), table(2)], eng, 3)


# ---- the entry point ----------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_bound_and_exported():
    import batched_cases as bc
    from mjmpc_amd import _lib
    header = bc.check_entry_points(["mjmpc_points", "mjmpc_points_motion", "mjmpc_points_tree", "mjmpc_points_orient"], abi=4)
    assert _lib.SIGNATURES["mjmpc_points_orient"] == _lib.SIGNATURES["mjmpc_points_tree"]
    assert "14 HOLD" in header and "15 ORIENTATION" in header and "2^-26" in header and "atan2(s, w)" in header


def test_bad_arguments_are_codes_and_messages():
    from mjmpc_amd import _lib
    lib = _lib.load()
    p = 64          # (never dereferenced: every call below is refused before anything is launched)

    def call(dtype=_lib.F64, N=1, d_obs=6, nq=2, nv=2, obs=p, prog=p, dofadr=p, n_rows=1, n_out=1, n_diff=0, n_levels=0, out=p):
        return lib.mjmpc_points_orient(dtype, N, d_obs, nq, nv, obs, prog, dofadr, n_rows, n_out, n_diff, n_levels, out, None)
    for kw in (dict(obs=None), dict(prog=None), dict(out=None), dict(dofadr=None), dict(N=0), dict(d_obs=0), dict(nq=7), dict(nq=0),
               dict(nv=0), dict(nv=-1), dict(nv=5), dict(nq=6, nv=1), dict(n_out=0), dict(n_out=17), dict(n_diff=17),
               dict(n_diff=-1), dict(n_rows=0), dict(n_rows=545), dict(n_rows=2, n_out=3), dict(dtype=7), dict(d_obs=8000),
               dict(n_levels=-1), dict(n_levels=5), dict(d_obs=7650, n_levels=4)):
        assert call(**kw) == -1, kw                 # MJMPC_E_BADARG
        assert lib.mjmpc_last_error().startswith(b"mjmpc_points_orient:"), (kw, lib.mjmpc_last_error())
    for kw, word in ((dict(n_levels=5), b"n_levels"), (dict(d_obs=7650, n_levels=4), b"saved frames"), (dict(dofadr=None), b"d_dofadr"),
                     (dict(nv=0), b"nv must be"), (dict(n_out=17), b"n_out must be"), (dict(n_rows=545), b"n_rows must be"),
                     (dict(dtype=7), b"unknown dtype"), (dict(obs=None), b"null pointer"), (dict(n_diff=17), b"n_diff must be"),
                     (dict(nq=7), b"nq must be"), (dict(N=0), b"N and d_obs")):
        call(**kw)
        assert word in lib.mjmpc_last_error(), (kw, lib.mjmpc_last_error())


def test_synthetic_programs_cover_what_they_must():
    """What tests/test_orient_gpu.py launches at the C entry, and a reference that notices each wrong interpreter."""
    import points_tile_cases as ptc
    cases = oc.synthetic_cases()
    for dtype in ("f64", "f32"):
        mine = [c for c in cases if c.dtype == dtype]
        assert {c.n_levels for c in mine} == {0, 2} and len({c.tile for c in mine if c.N <= c.tile + 1}) == 2
        for tile in {c.tile for c in mine if c.N <= c.tile + 1}:
            assert {c.N for c in mine if c.tile == tile and c.N <= c.tile + 1} == {1, tile, tile + 1}
    for c in cases:
        assert c.tile == cc.tree_tile_rows(c.dtype, c.d_obs, c.n_out, c.n_levels)
        assert cc.tree_lds_bytes(c.dtype, c.d_obs, c.n_out, c.n_levels, c.tile) <= ptc.LDS_BYTES
        rows = c.program[:c.n_rows]
        kinds = rows[:, 0].astype(int)
        assert c.n_out <= c.n_rows <= ptc.MAX_ROWS and np.sum(kinds == oc.HOLD) == 3
        slots = rows[kinds == oc.ORIENTATION][:, 2].astype(int)
        assert np.sum((slots < 0) | (slots >= c.n_out)) == 3 and set(c.slots) >= set(oc.EXACT_TAGS)
        assert kinds[6] == oc.ORIENTATION and rows[6, 11] == 1 and oc.HOLD not in kinds[:6]           # rel = 1 before any HOLD
        want80, interp64, b, settled = oc.synthetic_reference(c.name)
        assert settled.mean() >= 0.95 and ptc.excess_f64(interp64[settled], want80[settled], b)[0] <= 0.0

        def block(tag):
            return want80[:, 3 * c.slots[tag]:3 * c.slots[tag] + 3].astype(float)
        assert np.all(block("identity") == 0.0)
        assert np.allclose(block("w zero"), [np.pi, 0, 0], rtol=0, atol=1e-15)
        assert np.allclose(block("near pi"), [0, 0, oc.PI_MINUS], rtol=0, atol=1e-15)
        assert np.allclose(block("under"), [1.5 * oc.SMALL, 0, 0], rtol=1e-15, atol=0)
        assert np.allclose(block("over"), [0, -3.0 * oc.SMALL, 0], rtol=1e-15, atol=0)
        assert np.allclose(block("w negative"), [0, -2 * np.arctan2(0.6, 0.8), 0], rtol=0, atol=1e-15)
    c = oc.synthetic_case("orient-f64-l2")
    want80, interp64, b, settled = oc.synthetic_reference(c.name)
    for wrong in oc.WRONG:
        assert ptc.excess_f64(oc.synthetic_interpret(c, np.float64, wrong)[0][settled], want80[settled], b)[0] > 1e-6, wrong
    # the relative walk behind the centre of mass reads its own HOLD, and the HOLD leaves the sums alone
    at = c.slots
    assert np.abs(want80[:, 3 * at["relative"]:3 * at["relative"] + 3] - want80[:, 3 * at["after com"]:3 * at["after com"] + 3]).max() > 1e-3
