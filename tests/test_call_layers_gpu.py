"""The step path's host bookkeeping across composite calls (DESIGN.md sections 16 and 17: the enqueue layer and the call layer of
``simfire_hip.hip``).  After every call of a fixed script the test reads what the launch plan left on the handle -
``(last_launch_kind, last_launches, cell_layout)``, the arrival passes where recording is on, the window-updates counter where the
window kernel is forced - and compares the list with the one recorded on the library as it stood before the layers were separated
(``EXPECTED``, literals).  The same script on a twin handle in async mode, with one ``sync()`` at the end, must leave the same list,
the same state blobs and the same result rows.  Run with ``pytest -m gpu``."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# The smallest shapes at which each launch structure engages (plan_step of simfire_hip.hip): k_win needs H >= 64 and four vectors a
# row; run_team = 2 is honoured from two tile rows on, 136 rows are five.  "auto" runs the script a second time under set_fused(0).
SHAPES = {
    "auto": dict(H=64, W=64, md=4, then_fused0=True),
    "kwin": dict(H=64, W=64, md=4, tuning=dict(run_compact=2), window=True),
    "team": dict(H=136, W=64, md=4, tuning=dict(run_team=2)),
    "arrival": dict(H=64, W=64, md=2, arrival=True),
    "agents_u2": dict(H=64, W=64, md=4, agents=2),
    "agents_u3": dict(H=64, W=64, md=4, agents=3),
}
E, K = 2, 2


def _handle(c, async_mode):
    from simfire_amd.engine import FireEngine
    H, W = c["H"], c["W"]
    rng = np.random.default_rng(20261)
    eng = FireEngine(shape=(H, W), n_envs=E, max_fire_duration=c["md"], pixel_scale=30.0, update_rate=1.0, max_time=None,
                     attenuate_line_ros=True, diagonal_spread=True)
    if c.get("tuning"):
        eng.set_tuning(**c["tuning"])
    eng.set_rtable(rng.choice([3.0, 12.0, 30.0, 400.0], size=(8, H, W)))
    inits = np.array([[W // 2, H // 2], [W // 2 - 7, H // 2 + 5]], dtype=np.int32)
    eng.reset(inits)
    if c.get("arrival"):
        eng.enable_arrival(True)
    if c.get("window"):
        eng.enable_counters(True)
    if c.get("agents"):
        eng.agents_create(K, inits, n_updates=c["agents"], max_ticks=2, auto_reset=True)
        eng.agents_place([0, 1], np.array([[[3, 3], [W - 4, 3]], [[3, H - 4], [W - 4, H - 4]]], dtype=np.int32))
    if async_mode:
        eng.set_async(True)
    return eng


def _pair(eng, rec, label):
    eng.step(1)
    rec(label + " step")
    eng.status()
    rec(label + " status")


def _lines(c, n, x0):
    p = np.zeros((n, E, 2, 3), dtype=np.int32)
    for s in range(n):
        for e in range(E):
            p[s, e] = [(x0 + s, 2 + e, 3), (c["W"] - 1 - x0 - s, c["H"] - 3 - e, 4)]
    return p


def _script(eng, c, rec):
    """The calls, in the order of the issue's list; ``rec(label)`` after each."""
    import torch
    dst = torch.zeros((E, 8), dtype=torch.int32, device="cuda:0")

    def pair(label):
        _pair(eng, rec, label)

    def lines(n, x0):
        return _lines(c, n, x0)
    for i in range(4):                                   # 1. run(1) pairs until the single update runs resident
        pair(f"1.{i}")
    eng.step(1)                                          # 2. a look at the map behind a single update, then pairs again
    eng.fire_map(0)
    rec("2 step+fire_map")
    pair("2.a")
    pair("2.b")
    pair("2.c")
    eng.step(3)                                          # 3.
    rec("3 step(3)")
    eng.step_mitigated(lines(2, 1))                      # 4. control lines, untimed and timed
    rec("4 mitigated(2)")
    eng.step_mitigated(lines(3, 4), timed=True)
    rec("4 mitigated(3) timed")
    eng.step_mitigated(lines(1, 8))
    rec("4 mitigated(1)")
    pair("4.a")
    eng.run_delta(1, env=0)                              # 5.
    rec("5 run_delta(1)")
    eng.run_delta(1, env=0)
    rec("5 run_delta(1) again")
    pair("5.a")
    eng.rollout(2, dst.data_ptr())                       # 6.
    rec("6 rollout(2)")
    eng.rollout(1, dst.data_ptr())
    rec("6 rollout(1)")
    eng.rollout(1, dst.data_ptr())
    rec("6 rollout(1) again")
    pair("7.a")                                          # 7. a snapshot between two pairs is not a look
    eng.save_state([0, 1])
    rec("7 save_state")
    pair("7.b")
    eng.step(1)
    eng.save_state([1])
    rec("7 step+save_state")
    pair("7.c")
    eng.step(1)                                          # 8. the delta query is a look
    eng.fire_map_delta(0)
    rec("8 step+fire_map_delta")
    pair("8.a")
    pair("8.b")
    if c.get("agents"):                                  # 9.
        for t in range(3):
            a = torch.tensor([[(1 + t) + 5 * 1, 4 + 5 * 2], [2 + 5 * 3, (3 + t) % 5]], dtype=torch.int32, device="cuda:0")
            eng.agents_step(a)
            rec(f"9 tick {t}")
        pair("9.a")
        pair("9.b")
    eng.step_mitigated(lines(2, 12), timed=True)         # 10. pairs directly behind a call with control lines
    rec("10 mitigated(2) timed")
    pair("10.a")
    eng.step_mitigated(lines(5, 14))
    rec("10 mitigated(5)")
    pair("10.b")
    pair("10.c")
    pair("10.d")
    torch.cuda.synchronize()
    del dst


def _tail(eng, c, rec):
    """What the scatter + step pairs of ``step_mitigated`` leave behind, made visible: the pairs forced (``set_fused(0)``), untimed
    and timed - with recording on, a pass every ``max_fire_duration`` pairs and one behind the last show in the passes -, then the
    automatic mode again and run(1) pairs: how many it takes until the single update runs resident tells what the heuristic was
    left with (a call with control lines is no run(1) loop, and its last single update counts as one plain update)."""
    eng.set_fused(0)
    eng.step_mitigated(_lines(c, 5, 20))
    rec("11 pairs(5)")
    eng.step_mitigated(_lines(c, 3, 26), timed=True)
    rec("11 pairs(3) timed")
    eng.set_fused(-1)
    for i in range(5):
        _pair(eng, rec, f"11.{i}")


def _trace(name, async_mode):
    """(trace, state blobs, result rows, elapsed) of a shape's script."""
    c = SHAPES[name]
    eng = _handle(c, async_mode)
    trace = []

    def rec(label):
        t = (eng.last_launch_kind(), eng.last_launches(), eng.cell_layout())
        if c.get("arrival"):
            t += eng.arrival_passes()
        if c.get("window"):
            t += (eng.counters()["window_updates"],)
        trace.append((label,) + t)
    _script(eng, c, rec)
    if c.get("then_fused0"):
        eng.set_fused(0)
        rec("set_fused(0)")
        _script(eng, c, rec)
        eng.set_fused(-1)
    _tail(eng, c, rec)
    if async_mode:
        eng.sync()
    blobs = eng.save_state([0, 1])
    st, el = eng.status()
    eng.close()
    return trace, blobs, st, el


# Recorded on the library of the commit before the layers were separated (e56d15a), one MI355X.
EXPECTED = {'agents_u2': [(1, 0, 0), (1, 0, 0), (1, 0, 0), (1, 0, 0), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (1, 0, 0), (1, 0, 0),
                          (1, 0, 0), (1, 0, 0), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (1, 0, 0), (1, 0, 0), (1, 0, 0),
                          (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (1, 0, 0), (1, 0, 0), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1),
                          (2, 1, 1), (1, 0, 0), (1, 0, 0), (1, 0, 0), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (1, 0, 0), (1, 0, 0), (1, 0, 0),
                          (1, 0, 0), (1, 0, 0), (2, 1, 1), (2, 1, 1), (2, 1, 1), (1, 0, 0), (1, 0, 0), (2, 1, 1), (1, 0, 0), (1, 0, 0), (1, 0, 0),
                          (1, 0, 0), (2, 1, 1), (2, 1, 1), (0, 0, 0), (0, 0, 0), (1, 0, 0), (1, 0, 0), (1, 0, 0), (1, 0, 0), (2, 1, 1), (2, 1, 1),
                          (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1)],
 'agents_u3': [(1, 0, 0), (1, 0, 0), (1, 0, 0), (1, 0, 0), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (1, 0, 0), (1, 0, 0), (1, 0, 0),
               (1, 0, 0), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (1, 0, 0), (1, 0, 0), (1, 0, 0), (2, 1, 1), (2, 1, 1),
               (2, 1, 1), (2, 1, 1), (1, 0, 0), (1, 0, 0), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (1, 0, 0), (1, 0, 0),
               (1, 0, 0), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (1, 0, 0), (1, 0, 0), (1, 0, 0), (1, 0, 0),
               (2, 1, 1), (1, 0, 0), (1, 0, 0), (2, 1, 1), (1, 0, 0), (1, 0, 0), (1, 0, 0), (1, 0, 0), (2, 1, 1), (2, 1, 1), (0, 0, 0), (0, 0, 0),
               (1, 0, 0), (1, 0, 0), (1, 0, 0), (1, 0, 0), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1)],
 'arrival': [(1, 0, 0, 1, 1), (1, 0, 0, 1, 1), (1, 0, 0, 1, 2), (1, 0, 0, 1, 2), (2, 1, 1, 2, 2), (2, 1, 1, 2, 2), (2, 1, 1, 3, 2), (2, 1, 1, 3, 2),
             (2, 1, 1, 4, 2), (1, 0, 0, 4, 3), (1, 0, 0, 4, 3), (1, 0, 0, 4, 4), (1, 0, 0, 4, 4), (2, 1, 1, 5, 4), (2, 1, 1, 5, 4), (1, 1, 0, 6, 5),
             (2, 1, 1, 7, 5), (2, 2, 1, 9, 5), (2, 1, 1, 10, 5), (1, 0, 0, 10, 6), (1, 0, 0, 10, 6), (1, 0, 0, 10, 7), (2, 1, 1, 11, 7),
             (2, 1, 1, 12, 7), (2, 1, 1, 12, 7), (2, 1, 1, 13, 7), (1, 0, 0, 13, 8), (1, 0, 0, 13, 9), (2, 1, 1, 14, 9), (2, 1, 1, 14, 9),
             (2, 1, 1, 14, 9), (2, 1, 1, 15, 9), (2, 1, 1, 15, 9), (2, 1, 1, 16, 9), (1, 0, 0, 16, 10), (1, 0, 0, 16, 10), (1, 0, 0, 16, 11),
             (2, 1, 1, 17, 11), (2, 1, 1, 17, 11), (2, 1, 1, 18, 11), (2, 1, 1, 18, 11), (2, 1, 1, 19, 11), (1, 0, 0, 19, 12), (1, 0, 0, 19, 12),
             (2, 3, 1, 22, 12), (1, 0, 0, 22, 13), (1, 0, 0, 22, 13), (1, 0, 0, 22, 14), (1, 0, 0, 22, 14), (2, 1, 1, 23, 14), (2, 1, 1, 23, 14),
             (0, 0, 0, 23, 17), (0, 0, 0, 23, 19), (1, 0, 0, 23, 20), (1, 0, 0, 23, 20), (1, 0, 0, 23, 21), (1, 0, 0, 23, 21), (2, 1, 1, 24, 21),
             (2, 1, 1, 24, 21), (2, 1, 1, 25, 21), (2, 1, 1, 25, 21), (2, 1, 1, 26, 21), (2, 1, 1, 26, 21)],
 'auto': [(1, 0, 0), (1, 0, 0), (1, 0, 0), (1, 0, 0), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (1, 0, 0), (1, 0, 0), (1, 0, 0),
          (1, 0, 0), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (1, 0, 0), (1, 0, 0), (1, 0, 0), (2, 1, 1), (2, 1, 1),
          (2, 1, 1), (2, 1, 1), (1, 0, 0), (1, 0, 0), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (1, 0, 0), (1, 0, 0),
          (1, 0, 0), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (1, 0, 0), (1, 0, 0), (2, 1, 1), (1, 0, 0), (1, 0, 0), (1, 0, 0),
          (1, 0, 0), (2, 1, 1), (2, 1, 1), (2, 1, 1), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0),
          (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0),
          (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0),
          (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0),
          (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (1, 0, 0), (1, 0, 0), (1, 0, 0),
          (1, 0, 0), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1)],
 'kwin': [(1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 0, 0), (4, 1, 1, 2), (4, 1, 1, 2), (4, 1, 1, 4), (4, 1, 1, 4), (4, 1, 1, 6), (1, 0, 0, 6),
          (1, 0, 0, 6), (1, 0, 0, 6), (1, 0, 0, 6), (4, 1, 1, 8), (4, 1, 1, 8), (4, 1, 1, 14), (2, 1, 1, 14), (2, 1, 1, 14), (2, 1, 1, 14),
          (1, 0, 0, 14), (1, 0, 0, 14), (1, 0, 0, 14), (4, 2, 1, 16), (4, 2, 1, 18), (4, 2, 1, 18), (4, 2, 1, 22), (1, 0, 0, 22), (1, 0, 0, 22),
          (4, 2, 1, 24), (4, 2, 1, 24), (4, 2, 1, 24), (4, 2, 1, 26), (4, 2, 1, 26), (4, 2, 1, 28), (1, 0, 0, 28), (1, 0, 0, 28), (1, 0, 0, 28),
          (4, 2, 1, 30), (4, 2, 1, 30), (2, 1, 1, 30), (2, 1, 1, 30), (2, 1, 1, 30), (1, 0, 0, 30), (1, 0, 0, 30), (2, 1, 1, 30), (1, 0, 0, 30),
          (1, 0, 0, 30), (1, 0, 0, 30), (1, 0, 0, 30), (2, 1, 1, 30), (2, 1, 1, 30), (0, 0, 0, 30), (0, 0, 0, 30), (1, 0, 0, 30), (1, 0, 0, 30),
          (1, 0, 0, 30), (1, 0, 0, 30), (2, 1, 1, 30), (2, 1, 1, 30), (2, 1, 1, 30), (2, 1, 1, 30), (2, 1, 1, 30), (2, 1, 1, 30)],
 'team': [(1, 0, 0), (1, 0, 0), (1, 0, 0), (1, 0, 0), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (1, 0, 0), (1, 0, 0), (1, 0, 0),
          (1, 0, 0), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (1, 0, 0), (1, 0, 0), (1, 0, 0), (2, 1, 1), (2, 1, 1),
          (2, 1, 1), (2, 1, 1), (1, 0, 0), (1, 0, 0), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (1, 0, 0), (1, 0, 0),
          (1, 0, 0), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (1, 0, 0), (1, 0, 0), (2, 1, 1), (1, 0, 0), (1, 0, 0), (1, 0, 0),
          (1, 0, 0), (2, 1, 1), (2, 1, 1), (0, 0, 0), (0, 0, 0), (1, 0, 0), (1, 0, 0), (1, 0, 0), (1, 0, 0), (2, 1, 1), (2, 1, 1), (2, 1, 1),
          (2, 1, 1), (2, 1, 1), (2, 1, 1)]}


@pytest.mark.parametrize("name", list(SHAPES))
def test_trace_equals_the_recorded_one(name):
    sync_run = _trace(name, False)
    async_run = _trace(name, True)
    want = EXPECTED[name]
    got = [t[1:] for t in sync_run[0]]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (name, "call", i, sync_run[0][i][0], "got", g, "recorded", w)
    assert len(got) == len(want), (name, len(got), len(want))
    for i, (a, b) in enumerate(zip(async_run[0], sync_run[0])):
        assert a == b, (name, "async twin differs at call", i, a, b)
    assert len(async_run[0]) == len(sync_run[0])
    assert async_run[1].tobytes() == sync_run[1].tobytes(), (name, "state blobs of the twins differ")
    assert (async_run[2] == sync_run[2]).all() and async_run[3].tobytes() == sync_run[3].tobytes(), (name, "result rows of the twins differ")
