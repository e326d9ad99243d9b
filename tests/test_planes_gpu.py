"""The transitions of PlaneBook (simfire_amd/csrc/sf_planes.h) that the script of ``tests/test_call_layers_gpu.py`` does not reach, on
the GPU: a fire map loaded from outside, the per-cell kernel switched on and off with a count by ``k_counts`` in between, another
number of rows per band, the writable alias of the status plane, a reset of one environment, a new result sink, the closed loop.

After every call of the script the handle is compared with ``oracle.fire_dense.DenseOracle`` bit for bit - the result rows, elapsed,
every fire map, every ``burn`` plane - and, before that look (it converts to the row-major planes), the lab getters are read:
``cell_layout()`` and ``last_launch_kind()`` must be what ``EXPECTED`` lists.  Inside the closed loop only the rows ``loop_step``
returns are compared: any other call would end the loop.  Run with ``pytest -m gpu``."""
import numpy as np
import pytest

from oracle import fire_dense

pytestmark = pytest.mark.gpu

# Two environments of 64 x 64: the smallest shape at which both the window phase and the general loop of the resident launch engage.
# md = 6: sprite planes of two bytes, always the per-cell kernel - no kernel family to switch, no bands, no closed loop.
H, W, E = 64, 64, 2
CASES = {"md4": 4, "md6": 6}
INITS = [(30, 33), (21, 40)]


def _world(md):
    rng = np.random.default_rng(8800 + md)
    R8 = rng.choice([0.0, 3.0, 7.5, 12.0, 30.0], size=(8, H, W))
    R8[:, rng.random((H, W)) < 0.08] = 0.0
    kw = dict(shape=(H, W), n_envs=E, max_fire_duration=md, pixel_scale=20.0, update_rate=1.0, max_time=None, attenuate_line_ros=False,
              diagonal_spread=True)
    return R8, kw


def _same(eng, orc, tag):
    st_o, el_o = orc.status()
    st, el = eng.status()
    assert (st == st_o).all() and (el == el_o).all(), (tag, st, st_o)
    maps = eng.fire_maps()
    for e in range(E):
        assert (maps[e] == orc.fire_map(e)).all(), (tag, e, "fire map")
        assert (eng.burn(e) == orc.burn(e)).all(), (tag, e, "burn")


def _script(md):
    """The calls as (label, what to do with the engine, what to do with the oracle or None)."""
    import torch
    full = md == 4
    keep = {}                                            # tensors the handle writes to stay alive to the end

    def load_map(eng, orc):
        m = np.array(orc.fire_map(1), dtype=np.uint8)
        assert (m[6:9, 50:53] == 0).all()                # a second burning patch, away from the fire
        m[6:9, 50:53] = 1
        eng.load_fire_map(1, m)
        orc.load_fire_map(1, m)

    def both(name, *args):
        def call(eng, orc):
            getattr(eng, name)(*args)
            getattr(orc, name)(*args)
        return call

    def only(name, *args):
        return lambda eng, orc: getattr(eng, name)(*args)

    def other_band(eng, orc):
        rb = eng.geometry()["rows_per_band"]
        eng.set_rows_per_band(1 if rb != 1 else 2)
        assert eng.geometry()["rows_per_band"] != rb

    def alias(eng, orc):
        assert eng.cell_layout() == 0                    # (the look behind the last call left the row-major planes current)
        t = eng.fire_maps_torch()                        # nothing is written through it
        for e in range(E):
            assert (t[e].cpu().numpy() == orc.fire_map(e)).all(), (e, "alias")

    def new_sink(eng, orc):
        keep["sink"] = torch.full((E, 8), -1, dtype=torch.int32, device="cuda:0")
        eng.set_result_sink(keep["sink"].data_ptr())

    def rollout(eng, orc):
        keep["dst"] = torch.full((E, 8), -1, dtype=torch.int32, device="cuda:0")
        eng.rollout(2, keep["dst"].data_ptr())
        orc.step(2)
        st, _ = eng.status()
        assert (keep["sink"].cpu().numpy() == st).all() and (keep["dst"].cpu().numpy() == st).all()

    def loop_step(eng, orc):
        st, el = eng.loop_step()
        orc.step(1)
        st_o, el_o = orc.status()
        assert (st == st_o).all() and (el == el_o).all(), (st, st_o)

    def loop_refused(eng, orc):
        with pytest.raises(NotImplementedError):         # (SF_ENOTSUP: the closed loop needs the resident launch)
            eng.loop_start(0)

    s = [("1 reset", both("reset", np.array(INITS, dtype=np.int32))),
         ("2 step(3)", both("step", 3)),
         ("3 load_fire_map", load_map),
         ("4 status", only("status")),
         ("5 step(2)", both("step", 2))]
    if full:
        s.append(("6 set_generic(1)", only("set_generic", True)))
    s += [("7 step(2)", both("step", 2)),
          ("8 status", only("status"))]
    if full:
        s.append(("9 set_generic(0)", only("set_generic", False)))
    s.append(("10 step(1)", both("step", 1)))
    if full:
        s.append(("11 set_rows_per_band", other_band))
    s += [("12 step(2)", both("step", 2)),
          ("13 fire_maps_torch", alias),
          ("14 status", only("status")),
          ("15 reset_env", both("reset_env", 1, 40, 20)),
          ("16 step(3)", both("step", 3)),
          ("17 set_result_sink", new_sink),
          ("18 rollout(2)", rollout)]
    if full:
        s += [("19 loop_start", only("loop_start", 0)),
              ("20 loop_step", loop_step),
              ("20 loop_step again", loop_step),
              ("21 loop_stop", only("loop_stop"))]
    else:
        s.append(("19 loop_start refused", loop_refused))
    s += [("22 status", only("status")),
          ("23 step(2)", both("step", 2))]
    return s


def _run(name):
    """The script on a new handle and a new oracle; the list of (label, cell_layout, last_launch_kind) read behind every call."""
    from simfire_amd.engine import FireEngine
    md = CASES[name]
    R8, kw = _world(md)
    eng = FireEngine(**kw)
    eng.set_rtable(R8)
    orc = fire_dense.DenseOracle(**kw)
    orc.set_rtable(R8)
    trace = []
    for label, call in _script(md):
        call(eng, orc)
        trace.append((label, eng.cell_layout(), eng.last_launch_kind()))
        if not label.startswith(("19 loop_start", "20")) or md != 4:
            _same(eng, orc, (name, label))
    eng.set_result_sink(None)
    eng.close()
    return trace


# (cell_layout, last_launch_kind) behind every call, recorded on the parent's library (aa256eb, the handle's ten loose fields), one
# MI355X.  The blocked plane is current exactly behind the resident launches and the closed loop's calls.
EXPECTED = {
    "md4": [(1, -1), (1, 2), (0, 2), (0, 2), (1, 2), (0, 2), (0, 3), (0, 3), (0, 3), (0, 1), (0, 1), (1, 2), (0, 2), (0, 2), (0, 2), (1, 2), (0, 2),
            (1, 2), (1, 2), (1, 2), (1, 2), (1, 2), (0, 2), (1, 2)],
    "md6": [(0, -1)] + [(0, 3)] * 17,
}
# ... that is (md4; the per-cell kernel never uses it): the resident launches of step(n >= 2) and rollout, the closed loop from its start
# to its stop, and the first reset, which writes the blocked plane because the resident launch is what will step this handle.
BLOCKED_BEHIND = ("1 ", "2 ", "5 ", "12 ", "16 ", "18 ", "19 loop_start", "20 ", "21 ", "23 ")


@pytest.mark.parametrize("name", list(CASES))
def test_script_equals_the_oracle_and_the_recorded_layouts(name):
    trace = _run(name)
    print(name, [t[1:] for t in trace])
    want = EXPECTED[name]
    for t, w in zip(trace, want):
        assert t[1:] == w, (name, t, "recorded", w)
        assert t[1] == (1 if t[0].startswith(BLOCKED_BEHIND) and name == "md4" else 0), (name, t)
    assert len(trace) == len(want)
