"""Shared by tests/test_points_tiles_cpu.py and tests/test_points_tiles_gpu.py: synthetic launches of ``mjmpc_points`` and
``mjmpc_points_motion`` at the C entries - programs built from a seed in the row format of include/mjmpc_amd.h (no model, not
through ``cost_terms.points_program`` / ``motion_program``), observations with them, the launcher's tile rule restated, the
references (tests/motion_cases.py's interpreter in float64 and in 80-bit ``np.longdouble``) and the two criteria.

A case's nodes come from a skeleton - a sequence of joints with their qpos and dof addresses and their qpos0, as the jointed
bodies of one chain - of which every walk takes a stretch, with poses, axes and anchors of its own: walks share qpos entries as
paths with common ancestors do, and nq stays small beside 16 paths of 33 nodes.

The table (``cases()``) holds, for each of f64 and f32 and each of the two entries, every tile size 256 .. 1 at the narrowest
observation that reaches it with N = 2 rows + rows / 2 + 1 (three workgroups, the last ragged); N = 1, rows and rows + 1 at four
tile sizes with an odd d_obs; d_obs equal to the workgroup's 64 threads, twice that, and a d_aug of three times that; the
kernel's guards; and the largest programs the header allows."""
import dataclasses
import functools

import numpy as np

import motion_cases as mc

POINT, HINGE, SLIDE, BALL, FREE, DIFFERENCE, AXIS, VELOCITY, ANGULAR = 0, 1, 2, 3, 4, 5, 6, 7, 8
NQ_OF = {HINGE: 1, SLIDE: 1, BALL: 4, FREE: 7}
NV_OF = {HINGE: 1, SLIDE: 1, BALL: 3, FREE: 6}

# ---------------------------------------------------------------------------------------------------------- the launcher's rule
TILES = (256, 128, 64, 32, 16, 8, 4, 2, 1)
MAX_OUT, MAX_DIFF, MAX_NODES = 16, 16, 33
MAX_ROWS = MAX_OUT * (MAX_NODES + 1)            # 544
LDS_BYTES = 60 * 1024
WAVE = 64


def word(dtype):
    return 4 if dtype == "f32" else 8


def pitch(d_obs):
    return d_obs | 1


def lds_bytes(dtype, d_obs, n_out, rows):
    """The tile of ``rows`` rows, rounded up to a double, and their parked outputs."""
    return (rows * word(dtype) * pitch(d_obs) + 7) // 8 * 8 + rows * 8 * 3 * n_out


def widest(dtype, n_out):
    """The widest observation the launcher takes: one row and its outputs within the budget."""
    return (LDS_BYTES - 8 * 3 * n_out - 8) // word(dtype) - 1


def tile_rows(dtype, d_obs, n_out):
    """The rows of a workgroup's tile: 256 halved until the tile and its parked outputs fit 60 KiB."""
    assert 1 <= d_obs <= widest(dtype, n_out)
    rows = 256
    while lds_bytes(dtype, d_obs, n_out, rows) > LDS_BYTES:
        rows >>= 1
    return rows


def threads(rows):
    """wg = max(rows, 64): a workgroup never has less than a wavefront."""
    return max(rows, WAVE)


def narrowest(dtype, n_out, rows, at_least, odd=False):
    """The smallest d_obs >= ``at_least`` (odd, if asked) whose tile is ``rows`` rows; None if there is none."""
    for d in range(at_least, widest(dtype, n_out) + 1):
        if odd and d % 2 == 0:
            continue
        t = tile_rows(dtype, d, n_out)
        if t == rows:
            return d
        if t < rows:
            return None
    return None


def refusal(c):
    """The launcher's documented argument checks (include/mjmpc_amd.h) over a case: None, or what it refuses."""
    if c.N < 1 or c.d_obs < 1:
        return "N or d_obs below 1"
    if not 1 <= c.nq <= c.d_obs:
        return "nq outside 1 .. d_obs"
    if not 1 <= c.n_out <= MAX_OUT:
        return "n_out outside 1 .. 16"
    if not 0 <= c.n_diff <= MAX_DIFF:
        return "n_diff outside 0 .. 16"
    if not c.n_out <= c.n_rows <= MAX_ROWS:
        return "n_rows outside n_out .. 544"
    if c.d_obs > widest(c.dtype, c.n_out):
        return "a row that does not fit the tile with its outputs"
    if c.entry == "motion" and (c.nv < 1 or c.nq + c.nv > c.d_obs or c.dofadr is None):
        return "nv below 1, nq + nv above d_obs or no dofadr"
    return None


# ---------------------------------------------------------------------------------------------------------- the programs
@dataclasses.dataclass
class Case:
    name: str
    entry: str                      # "points": mjmpc_points, "motion": mjmpc_points_motion
    dtype: str                      # "f64" / "f32": the storage type of the rows
    tile: int                       # the rows of a workgroup's tile the table claims
    N: int
    d_obs: int
    nq: int
    nv: int
    program: np.ndarray             # float64 [n_rows + n_diff][16]
    dofadr: np.ndarray              # int32 [n_rows] (motion; None for points)
    n_rows: int
    n_out: int
    n_diff: int
    nodes: int                      # the longest walk's
    obs: np.ndarray                 # [N][d_obs] in the storage type
    tags: frozenset
    deep: bool = False

    @property
    def d_aug(self):
        return self.d_obs + 3 * self.n_out + 3 * self.n_diff

    @property
    def base(self):
        """The first entry of a row the kernel only copies."""
        return self.nq + (self.nv if self.entry == "motion" else 0)


def _unit(rs, n):
    v = rs.standard_normal(n)
    return v / np.linalg.norm(v)


def _offset(rs):
    """A vector of length 0.05 .. 0.2."""
    return rs.uniform(0.05, 0.2) * _unit(rs, 3)


def skeleton(rs, kinds):
    """-> ([(kind, qpos address, dof address, qpos0)], nq, nv): the joints of one chain, addresses in MuJoCo's layout."""
    out, nq, nv = [], 0, 0
    for i, kind in enumerate(kinds):
        assert kind in NQ_OF and (kind != FREE or i == 0)
        out.append((kind, nq, nv, rs.uniform(0.2, 0.9) * rs.choice([-1.0, 1.0])))
        nq, nv = nq + NQ_OF[kind], nv + NV_OF[kind]
    return out, nq, nv


def node_row(rs, joint):
    """A node row: the body 0.1 or so from the frame before it, turned anyhow; a unit axis; an anchor 0.1 or so off."""
    kind, adr, _, qpos0 = joint
    row = np.zeros(16)
    row[0], row[1] = kind, adr
    if kind == FREE:
        return row                                      # (a free joint replaces the frame: nothing else is read)
    row[2] = qpos0 if kind in (HINGE, SLIDE) else 0.0
    row[3:6] = _offset(rs)
    row[6:10] = _unit(rs, 4)
    if kind in (HINGE, SLIDE):
        row[10:13] = _unit(rs, 3)
    if kind in (HINGE, BALL):
        row[13:16] = _offset(rs)
    return row


def program_of(rs, joints, walks, differences, entry):
    """``walks``: [(first, last, [(closing kind, slot)])] - the node rows of joints[first:last], then the closing rows, all but
    the last keeping the frame.  For ``mjmpc_points`` every closing row is {0, 0, 0, x, y, z}: the slots are the order.
    -> (program, dofadr, n_rows, the longest walk's nodes)."""
    rows, dofadr = [], []
    for first, last, closings in walks:
        assert last - first <= MAX_NODES and closings
        for joint in joints[first:last]:
            rows.append(node_row(rs, joint))
            dofadr.append(joint[2])
        for i, (kind, slot) in enumerate(closings):
            row = np.zeros(16)
            if entry == "motion":
                row[0], row[1], row[2] = kind, float(i + 1 < len(closings)), slot
            else:
                assert kind == POINT and len(closings) == 1
            if kind != ANGULAR:
                row[3:6] = _unit(rs, 3) if kind == AXIS else _offset(rs)
            rows.append(row)
            dofadr.append(0)
    n_rows = len(rows)
    for a, b in differences:
        rows.append(np.array([DIFFERENCE, a, b] + [0.0] * 13))
    return (np.array(rows), np.array(dofadr, np.int32) if entry == "motion" else None, n_rows,
            max(last - first for first, last, _ in walks))


# ---------------------------------------------------------------------------------------------------------- the observations
def _special_words(dtype):
    """Bit patterns the copy must carry as they are: signed zeros, infinities, denormals, NaNs with payloads of their own
    (quiet and signalling, of either sign)."""
    if dtype == "f32":
        bits = [0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x00000001, 0x80000001, 0x007fffff, 0x00012345,
                0x7fc00000, 0x7fc00001, 0xffc0beef, 0x7f800001, 0xffa5a5a5, 0x7fffffff]
        return np.array(bits, np.uint32)
    bits = [0x0000000000000000, 0x8000000000000000, 0x7ff0000000000000, 0xfff0000000000000, 0x0000000000000001,
            0x8000000000000001, 0x000fffffffffffff, 0x0000000123456789, 0x7ff8000000000000, 0x7ff8000000000001,
            0xfff80000deadbeef, 0x7ff0000000000001, 0xfff5a5a5a5a5a5a5, 0x7fffffffffffffff]
    return np.array(bits, np.uint64)


SPECIAL_CLASSES = ("signed zero", "infinity", "denormal", "nan")


def special_classes(c):
    """Which of SPECIAL_CLASSES the copied entries of a case hold, and how many distinct NaN patterns."""
    x = c.obs[:, c.base:]
    seen = set()
    if np.any((x == 0) & np.signbit(x)) and np.any((x == 0) & ~np.signbit(x)):
        seen.add("signed zero")
    if np.any(np.isposinf(x)) and np.any(np.isneginf(x)):
        seen.add("infinity")
    if np.any((x != 0) & (np.abs(x) < np.finfo(x.dtype).tiny)):
        seen.add("denormal")
    nans = np.unique(x.view(np.uint32 if c.dtype == "f32" else np.uint64)[np.isnan(x)])
    if len(nans) >= 2:
        seen.add("nan")
    return seen, len(nans)


def observations(rs, c_dtype, N, d_obs, joints, nq, nv, entry):
    """[N][d_obs] in the storage type: hinge and slide entries up to pi about qpos0; quaternions of norm 1, 0.5 and 3 in turn;
    qvel of order 1; behind them the special words, turned round by one from row to row, then plain numbers."""
    obs = rs.standard_normal((N, d_obs))
    scales = (1.0, 0.5, 3.0)
    for j, (kind, adr, _, qpos0) in enumerate(joints):
        if kind in (HINGE, SLIDE):
            obs[:, adr] = qpos0 + rs.uniform(-np.pi, np.pi, N)
            continue
        if kind == FREE:
            obs[:, adr:adr + 3] = 0.3 * rs.standard_normal((N, 3))
            adr += 3
        quat = rs.standard_normal((N, 4))
        quat /= np.linalg.norm(quat, axis=1, keepdims=True)
        obs[:, adr:adr + 4] = quat * np.array([scales[(n + j) % 3] for n in range(N)])[:, None]
    obs = obs.astype(np.float32 if c_dtype == "f32" else np.float64)
    base = nq + (nv if entry == "motion" else 0)
    words = _special_words(c_dtype)
    k = min(len(words), d_obs - base)
    if k > 0:
        view = obs.view(words.dtype)
        for n in range(N):
            view[n, base:base + k] = np.roll(words, -n)[:k]
    return obs


# ---------------------------------------------------------------------------------------------------------- the table
SMALL = (HINGE, BALL)                                       # nq 5, nv 4: with PAD, the 23 entries a 256-row f64 tile takes
MEDIUM = (FREE, HINGE, BALL, SLIDE, HINGE, HINGE)           # nq 15, nv 13
PAD = 14                                                    # entries behind qpos (and qvel) a case keeps: the special words


def _full_kinds(rs):
    """33 joints: a free root, five ball joints, hinges and slides."""
    kinds = [FREE] + [HINGE if rs.uniform() < 0.7 else SLIDE for _ in range(32)]
    for i in (3, 9, 16, 24, 32):
        kinds[i] = BALL
    return tuple(kinds)


def _shape(which, entry, rs):
    """-> (kinds, walks, differences, n_out) of a program shape."""
    closing = (POINT, AXIS, VELOCITY, ANGULAR)
    if which == "small":
        if entry == "points":
            return SMALL, [(0, 2, [(POINT, 0)]), (0, 1, [(POINT, 1)])], [(0, 1)], 2
        return SMALL, [(0, 2, [(POINT, 1), (VELOCITY, 0)])], [(1, 0)], 2
    if which == "medium":
        if entry == "points":
            walks = [(0, 6, [(POINT, 0)]), (1, 4, [(POINT, 1)]), (0, 3, [(POINT, 2)]), (1, 6, [(POINT, 3)]), (0, 1, [(POINT, 4)])]
            return MEDIUM, walks, [(0, 1), (3, 2), (4, 4)], 5
        walks = [(0, 6, [(POINT, 3), (VELOCITY, 0), (ANGULAR, 4)]), (1, 5, [(AXIS, 1)]), (0, 3, [(VELOCITY, 2)])]
        return MEDIUM, walks, [(0, 2), (3, 3), (4, 1)], 5
    if which == "wide":                                 # 16 outputs on the medium chain
        if entry == "points":
            walks = [(i % 2, i % 2 + 1 + i % 5, [(POINT, i)]) for i in range(16)]
        else:
            slots = [(7 * i + 3) % 16 for i in range(16)]
            walks, k = [], 0
            for (first, last), n in zip(((0, 6), (1, 5), (0, 3), (1, 6), (0, 1), (1, 3)), (4, 3, 3, 2, 2, 2)):
                walks.append((first, last, [(closing[(k + i) % 4], slots[k + i]) for i in range(n)]))
                k += n
        return MEDIUM, walks, [(i, (i + 3) % 16) for i in range(6)], 16
    kinds = _full_kinds(rs)
    differences = [(i, (i + 5) % 16) for i in range(15)] + [(7, 7)]
    if which == "full":
        # 16 walks of 33 nodes and a closing row each: 544 rows.  One walk starts at the free joint; the others cannot (a free
        # joint stands first), so their 33 nodes are the chain behind it and its last joint once more
        kinds = kinds + (HINGE,)
        walks = [(0, 33, [(closing[0], 0)])] + [(1, 34, [(closing[i % 4] if entry == "motion" else POINT, i)]) for i in range(1, 16)]
        return kinds, walks, differences, 16
    assert which == "shared" and entry == "motion"
    # 15 walks of 33 nodes and one of 30, 19 closing rows: 544 rows.  The first walk carries four closing rows, one of each
    # kind; the slots run backwards; 5 and 10 are named by no row; five rows name a slot outside and write nothing
    kinds = kinds + (HINGE,)
    walks = [(0, 33, [(POINT, 15), (AXIS, 14), (VELOCITY, 13), (ANGULAR, 12)])]
    walks += [(1, 31 if s == 9 else 34, [(closing[i % 4], s)]) for i, s in enumerate((11, 9, 8, 7, 6, 4, 3, 2, 1, 0))]
    walks += [(1, 34, [(closing[i % 4], s)]) for i, s in enumerate((16, -1, 99, 1 << 20, -3))]
    differences = differences[:13] + [(5, 15), (14, 10), (10, 5)]
    return kinds, walks, differences, 16


def make_case(name, seed, entry, dtype, which, tile, n, d_obs=None, odd=False, tags=(), wild=False):
    """A case whose tile is ``tile`` rows: at the narrowest d_obs that reaches it (behind qpos, qvel and PAD special words)
    unless ``d_obs`` is given.  ``n``: N, or a function of the tile's rows."""
    rs = np.random.RandomState(seed)
    kinds, walks, differences, n_out = _shape(which, entry, rs)
    joints, nq, nv = skeleton(rs, kinds)
    program, dofadr, n_rows, nodes = program_of(rs, joints, walks, differences, entry)
    base = nq + (nv if entry == "motion" else 0)
    if d_obs is None:
        d_obs = narrowest(dtype, n_out, tile, base + PAD, odd)
        assert d_obs is not None, name
    N = n(tile) if callable(n) else n
    tags = set(tags)
    if wild:
        tags |= _go_wild(program, dofadr, n_rows, n_out, nq, nv, entry)
    obs = observations(rs, dtype, N, d_obs, joints, nq, nv, entry)
    return Case(name=name, entry=entry, dtype=dtype, tile=tile, N=N, d_obs=d_obs, nq=nq, nv=nv, program=program, dofadr=dofadr,
                n_rows=n_rows, n_out=n_out, n_diff=len(differences), nodes=nodes, obs=obs, tags=frozenset(tags),
                deep=which in ("full", "shared"))


def _go_wild(program, dofadr, n_rows, n_out, nq, nv, entry):
    """The medium program with addresses and indices the kernel must hold inside: the ball joint's address two short of nq's
    end in one walk and far past it in another, the free joint's straddling nq's end, a hinge's below 0; dof addresses past nv
    and below 0; a closing row with a slot outside (motion) or behind the last point (points: one walk more than n_points);
    differences with a == b, an index below 0 and one above n_out - 1, and under motion one that reads a slot no row names."""
    tags = set()
    node = [k for k in range(n_rows) if program[k, 0] in NQ_OF]
    balls = [k for k in node if program[k, 0] == BALL]
    frees = [k for k in node if program[k, 0] == FREE]
    hinges = [k for k in node if program[k, 0] == HINGE]
    assert len(balls) >= 2 and len(frees) >= 2 and len(hinges) >= 3
    program[balls[0], 1], program[balls[1], 1] = nq - 2, nq + 1000
    program[frees[1], 1] = nq - 5
    program[hinges[1], 1] = -4
    tags |= {"ball past nq", "free past nq"}
    if entry == "motion":
        dofadr[balls[0]], dofadr[frees[1]], dofadr[hinges[2]], dofadr[hinges[0]] = nv - 1, nv - 4, nv + 77, -9
        tags.add("dof past nv")
        closing = [k for k in range(n_rows) if program[k, 0] not in NQ_OF]
        program[closing[1], 2] = n_out + 3              # the velocity that named slot 0: now slot 0 is named by no row
        program[closing[3], 2] = -1
        program[n_rows:, 1:3] = [[0, 2], [3, 3], [-2, n_out + 5]]
        tags |= {"slot outside", "difference of an unnamed slot"}
    else:
        program[n_rows:, 1:3] = [[0, 1], [3, 3], [-2, n_out + 5]]
        tags.add("slot outside")                        # (cases() takes one off n_points: the last walk's point)
    tags |= {"a == b", "difference index below 0", "difference index above n_out - 1"}
    return tags


def _ragged(rows):
    return 2 * rows + rows // 2 + 1


@functools.lru_cache(maxsize=None)
def cases():
    out, seed = [], 1000
    for dtype in ("f64", "f32"):
        for entry in ("points", "motion"):
            for tile in TILES:                          # every tile size: three workgroups, the last ragged
                seed += 1
                which = "small" if tile == 256 else "medium"
                out.append(make_case("%s-%s-t%d" % (entry, dtype, tile), seed, entry, dtype, which, tile, _ragged,
                                     tags=("ragged", "narrowest")))
        for entry, tile in ((e, t) for t in (256, 64, 16, 2) for e in ("points", "motion")):       # N's edges, odd d_obs
            for tag, n in (("N = 1", 1), ("N = rows", lambda r: r), ("N = rows + 1", lambda r: r + 1)):
                seed += 1
                which = "small" if tile == 256 else "medium"
                out.append(make_case("%s-%s-t%d-%s" % (entry, dtype, tile, tag.replace(" ", "")), seed, entry, dtype, which, tile,
                                     n, odd=True, tags=(tag,)))
        for entry in ("points", "motion"):              # the widths' edges, all at 64 threads
            n_extra = 3 * 5 + 3 * 3
            # (64 f32 entries with five outputs make a tile of 128 rows and as many threads; with sixteen, one of 64)
            for tag, d_obs, which in (("d_obs == wg", WAVE, "medium" if dtype == "f64" else "wide"),
                                      ("d_obs a multiple of wg", 2 * WAVE, "medium"),
                                      ("d_aug a multiple of wg", 3 * WAVE - n_extra, "medium"),
                                      ("odd d_obs above wg", 2 * WAVE + 3, "medium")):
                seed += 1
                tile = tile_rows(dtype, d_obs, 16 if which == "wide" else 5)
                out.append(make_case("%s-%s-%s" % (entry, dtype, tag.replace(" ", "_")), seed, entry, dtype, which, tile,
                                     _ragged, d_obs=d_obs, tags=(tag,)))
            seed += 1                                   # the guards
            c = make_case("%s-%s-wild" % (entry, dtype), seed, entry, dtype, "medium", 32, _ragged, wild=True, tags=("wild",))
            if entry == "points":                       # the last walk's point stands behind the last of n_points
                c = dataclasses.replace(c, n_out=c.n_out - 1, tile=tile_rows(dtype, c.d_obs, c.n_out - 1))
            out.append(c)
            for which in ("full", "shared")[:2 if entry == "motion" else 1]:       # the largest programs
                seed += 1
                tile = tile_rows(dtype, narrowest_full(dtype, entry), 16)
                out.append(make_case("%s-%s-%s" % (entry, dtype, which), seed, entry, dtype, which, tile, _ragged,
                                     tags=(which, "ragged")))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def narrowest_full(dtype, entry):
    """The d_obs of the full programs: their qpos, qvel and PAD entries more."""
    kinds = _full_kinds(np.random.RandomState(0)) + (HINGE,)
    nq, nv = sum(NQ_OF[k] for k in kinds), sum(NV_OF[k] for k in kinds)
    return nq + (nv if entry == "motion" else 0) + PAD


def case(name):
    return {c.name: c for c in cases()}[name]


def names():
    return [c.name for c in cases()]


# ---------------------------------------------------------------------------------------------------------- the references
def interpret(c, dtype, wrong=None):
    """The case's new entries [N][3 n_out + 3 n_diff] in ``dtype`` arithmetic from the rows as stored, widened (exactly)."""
    obs = c.obs[:, :c.base].astype(dtype)
    motion = c.entry == "motion"
    return mc.interpret(c.program, c.n_rows, c.dofadr, c.n_out, obs[:, :c.nq], obs[:, c.nq:c.nq + c.nv] if motion else None,
                        wrong=wrong, dtype=dtype, slots_in_order=not motion, guards=True)


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (want80, interp64, bound): made once for all tests, read only."""
    c = case(name)
    want80, interp64 = interpret(c, np.longdouble), interpret(c, np.float64)
    assert want80.dtype == np.longdouble and interp64.dtype == np.float64 and np.all(np.isfinite(want80))
    b = bound(c, want80, interp64)
    for a in (want80, interp64):
        a.setflags(write=False)
    return want80, interp64, b


MARGIN = 32


def bound(c, want80, interp64):
    """32 times the float64 interpreter's own worst rounding over the case's rows - the margin: the kernel composes
    quaternions where the interpreter composes matrices, and its sincos, rsqrt and sqrt may each be an ulp or two off per node -,
    and no less than (nodes + 2) 2^-52 max(1, max |want80|)."""
    own = float(np.abs(interp64.astype(np.longdouble) - want80).max())
    floor = (c.nodes + 2) * 2.0 ** -52 * max(1.0, float(np.abs(want80).max()))
    return max(MARGIN * own, floor)


def excess_f64(got, want80, b):
    """max (|got - want80| - bound): <= 0 where the f64 criterion holds; also the worst error."""
    err = np.abs(np.asarray(got).astype(np.longdouble) - want80)
    return float((err - b).max()), float(err.max())


def excess_f32(got, want80, b):
    """max (|got - want80| - (ulp32(want80) / 2 + bound)): the header's "rounded once"; also the worst error, and the worst in
    units of ulp32(want80)."""
    err = np.abs(np.asarray(got).astype(np.longdouble) - want80)
    ulp = np.spacing(np.abs(want80).astype(np.float32)).astype(np.longdouble)
    return float((err - 0.5 * ulp - b).max()), float(err.max()), float((err / ulp).max())
