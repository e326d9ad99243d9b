"""The step path of the resident launch after NOTEBOOK.md 5.18: lists of one round are dealt out by wave number (no cursor), the kernel
whose teams grow inside the launch - k_run<1, 0, 1, 0, 2>, bench.py's - reads its argument block two ways, runs the batch loop unrolled
by two and carries no statistics; a handle with the counters on launches k_run<1, 0, 1, 0, 3>, the same kernel with them.  None of that may change a
result: every world below is stepped in ONE call and compared with oracle.fire_dense.DenseOracle bit for bit - the result block, every
fire map, every burn_amounts plane.

Which kernel a call takes is the host's decision (simfire_hip.hip: plan_segment, join_geometry) and is asserted per world:
  * the kernel whose teams grow: at least two environments, at least 192 updates in the call, one-word rows, at least two tile rows,
    no control lines inside the launch, no launch-geometry knob set by hand - and NOT in dense mode;
  * dense mode (`set_dense`: every vector is on the list, so the list's length is known in closed form) and a vector capacity set by
    hand take the plain kernel k_run<1, 0, 1, 0, 0>, with one wave per 64 rows.  Its loop over the list is the same source; the
    one-round rule needs 16 waves, i.e. more than 960 rows - the issue's dense worlds of 64 .. 136 rows stay on the cursor (2 - 3 waves),
    so three dense worlds of 968 .. 1024 rows are added: 16 batches exactly, 16 batches with a short last one, and two rounds.

The reference of a world is computed once (the oracle alone, seconds on a CPU) and shared by the cases that step it; it is read-only."""
import numpy as np
import pytest

from oracle import fire_dense

pytestmark = pytest.mark.gpu

KW = dict(max_fire_duration=4, pixel_scale=20.0, update_rate=1.0, max_time=None, attenuate_line_ros=False, diagonal_spread=True)

# name -> (H, W, environments, updates, dense, seed)
WORLDS = {
    # lists around the one-round limit of a 16-wave workgroup (1024 vectors): the issue's three dense worlds ...
    "dense_128x128": (128, 128, 8, 200, True, 11),       # 1024 vectors: 16 batches of 64
    "dense_136x128": (136, 128, 8, 200, True, 12),       # 1088 vectors: 17 batches
    "dense_64x128": (64, 128, 8, 200, True, 13),         # 512 vectors
    # ... and three whose plain kernel has the 16 waves the rule asks for
    "dense_1024x16": (1024, 16, 2, 200, True, 14),       # 1024 vectors, one per row: one round, every wave a full batch
    "dense_968x16": (968, 16, 2, 200, True, 15),         # 968 vectors: one round, the last batch short, no second look at the cursor
    "dense_1000x32": (1000, 32, 2, 200, True, 16),       # 2000 vectors: two rounds, handed out by the cursor
    # pitch padding in the last vector (W = 120), and the same shapes as above with the list the fire makes
    "fire_128x128": (128, 128, 8, 200, False, 21),
    "fire_136x128": (136, 128, 8, 200, False, 22),
    "fire_64x128": (64, 128, 8, 200, False, 23),
    "fire_128x120": (128, 120, 8, 200, False, 24),
    # teams that form: some fires die early on patches that do not burn, their workgroups join the others
    "teams_256x256": (256, 256, 16, 260, False, 31),
}
_REF = {}


def _world(name):
    H, W, E, n, dense, seed = WORLDS[name]
    rng = np.random.default_rng(8800 + seed)
    R8 = rng.choice([0.0, 3.0, 7.5, 12.0, 30.0], size=(8, H, W))
    R8[:, rng.random((H, W)) < 0.08] = 0.0
    inits = [(int(rng.integers(W // 4, W - W // 4)) if W >= 64 else int(rng.integers(W)), int(rng.integers(H // 4, H - H // 4))) for _ in range(E)]
    if name.startswith("teams"):
        # every other fire starts on an island: a ring that does not burn five cells out (the table's entry of the TARGET cell is what counts)
        y, x = np.mgrid[0:H, 0:W]
        for e in range(0, E, 2):
            ix, iy = inits[e] = (20 + 13 * e, 30 + 12 * e)
            d = np.maximum(np.abs(x - ix), np.abs(y - iy))
            R8[:, (d >= 4) & (d <= 6)] = 0.0
        for e in range(1, E, 2):                                   # (the others beside an island, clear of every ring)
            inits[e] = (inits[e - 1][0] + 30, inits[e - 1][1] - 15)
    return dict(H=H, W=W, E=E, n=n, dense=dense, R8=R8, inits=inits, kw=dict(KW, shape=(H, W), n_envs=E))


def _reference(name):
    """(status rows, elapsed, fire maps, burn planes) of the world after its one call - the oracle alone, once per world, read-only."""
    if name not in _REF:
        w = _world(name)
        o = fire_dense.DenseOracle(**w["kw"])
        o.set_rtable(w["R8"])
        o.reset(w["inits"])
        o.step(w["n"], 8)
        st, el = o.status()
        out = (np.array(st), np.array(el), [np.array(o.fire_map(e)) for e in range(w["E"])], [np.array(o.burn(e)) for e in range(w["E"])])
        for a in (out[0], out[1], *out[2], *out[3]):
            a.setflags(write=False)
        _REF[name] = out
    return _REF[name]


def _engine(name, counters, **tuning):
    from simfire_amd.engine import FireEngine
    w = _world(name)
    eng = FireEngine(**w["kw"])
    eng.set_rtable(w["R8"])
    eng.reset(w["inits"])
    eng.set_fused(2)
    if w["dense"]:
        eng.set_dense(True)
    if tuning:
        eng.set_tuning(**tuning)
    if counters:
        eng.enable_counters(True)
        eng.counters(reset=True)
    return eng, w


def _same(eng, name):
    st_o, el_o, maps_o, burn_o = _reference(name)
    st, el = eng.status()
    assert (st == st_o).all() and (el == el_o).all(), name
    maps = eng.fire_maps()
    for e in range(len(maps_o)):
        assert (maps[e] == maps_o[e]).all(), (name, e, "fire map")
        assert (eng.burn(e) == burn_o[e]).all(), (name, e, "burn")


def _check_counters(eng, name, w):
    """The statistics as the parent counted them.  ignitions: every cell that caught fire in the call - BURNING or BURNED at the end,
    less the one ignition cell per environment the reset lit.  vectors (dense mode, no window phase): every update that was made visited
    every vector of the grid, rows x pitch / 16."""
    st_o = _reference(name)[0]
    c = eng.counters()
    lit = int(st_o[:, 3].sum() + st_o[:, 4].sum()) - w["E"]
    print(name, "counters:", c, "| cells lit in the call:", lit)
    assert c["ignitions"] == lit, (name, c["ignitions"], lit)
    assert c["vectors"] > 0 and c["frontier_walks"] > 0 and c["frontier_items"] >= lit and c["active_cell_updates"] >= lit
    if w["dense"]:
        pitch = eng.fire_map_device()[1]
        n_vec = w["H"] * (pitch // 16)
        updates = int(st_o[:, 1].sum())
        print(name, "vectors per update:", n_vec, "updates made:", updates)
        assert c["vectors"] == n_vec * updates, (name, c["vectors"], n_vec, updates)


def _grew(eng, w):
    """The kernel whose teams grow ran: one resident launch, every environment with a team of 1 .. 4 (zeros: not a team launch)."""
    sizes = eng.team_sizes()
    print("team sizes:", sizes.tolist())
    return eng.last_launch_kind() == 2 and eng.last_launches() == 1 and sizes.min() >= 1 and sizes.max() <= 4


def test_the_references_differ_from_their_start():
    """The worlds do something: fires spread, and in the team world some go out early (their workgroups are what joins)."""
    for name in WORLDS:
        st = _reference(name)[0]
        assert (st[:, 3] + st[:, 4]).sum() > 20 * st.shape[0], name
    st = _reference("teams_256x256")[0]
    assert (st[0::2, 0] == 0).all() and (st[0::2, 1] < 60).all(), st[0::2, :2]       # the islands: out within a few dozen updates
    assert (st[1::2, 1] == 260).all(), st[1::2, :2]                                    # the others: every update of the call


@pytest.mark.parametrize("counters", [False, True])
@pytest.mark.parametrize("name", [n for n in WORLDS if n.startswith("dense")])
def test_dense_lists_around_one_round(name, counters):
    """Every vector on the list: 512 .. 2000 vectors on 2 .. 16 waves (the plain kernel: the host does not offer teams in dense mode)."""
    eng, w = _engine(name, counters, run_window=-1)
    eng.step(w["n"])
    assert eng.last_launch_kind() == 2 and eng.last_launches() == 1
    assert eng.team_sizes().max() == 0                                                 # (see the module's text)
    _same(eng, name)
    if counters:
        _check_counters(eng, name, w)


@pytest.mark.parametrize("counters", [False, True])
@pytest.mark.parametrize("name", [n for n in WORLDS if n.startswith("fire")])
def test_lists_the_fire_makes(name, counters):
    """The same shapes, and a grid whose last vector is part pitch padding, on the kernel whose teams grow."""
    eng, w = _engine(name, counters)
    eng.step(w["n"])
    print(name, "launch kind", eng.last_launch_kind(), "launches", eng.last_launches())
    assert _grew(eng, w)
    _same(eng, name)
    if counters:
        _check_counters(eng, name, w)


@pytest.mark.parametrize("counters", [False, True])
@pytest.mark.parametrize("placement", [0, 1, 2])
@pytest.mark.parametrize("recut", [4, 7])
def test_teams_form_cut_and_join(recut, placement, counters):
    """16 environments, 260 updates, the bands cut anew every 4 / 7 updates (SF_TUNE_RUN_SEGMENT = twice that), every free workgroup
    joins whatever runs (SF_TUNE_RUN_JOIN < 0), members from one XCD / from anywhere / from one XCD but handed off as if apart."""
    name = "teams_256x256"
    eng, w = _engine(name, counters, run_join=-2, run_segment=2 * recut, team_placement=placement)
    eng.step(w["n"])
    assert _grew(eng, w)
    sizes, log = eng.team_sizes(), eng.join_log()
    assert (sizes > 1).any(), sizes                                                    # teams did form ...
    grown = log[log[:, 2] != 255]
    assert len(grown) > 0 and (grown[:, 1] % recut == 0).all(), grown[:8]              # ... at the cuts
    _same(eng, name)
    if counters:
        _check_counters(eng, name, w)
        assert eng.counters()["team_boundaries"] > 0


@pytest.mark.parametrize("counters", [False, True])
def test_chunked_dense_list(counters):
    """17 batches through a list of 256 entries: five chunks per update, the cursor reset between them (a capacity set by hand: the
    plain kernel)."""
    name = "dense_136x128"
    eng, w = _engine(name, counters, run_window=-1, run_vcap=256)
    eng.step(w["n"])
    assert eng.last_launch_kind() == 2 and eng.last_launches() == 1
    _same(eng, name)
    if counters:
        _check_counters(eng, name, w)
