#!/usr/bin/env python3
"""Generate ``ignite_*.npz`` from the REAL reference: trajectories of ``RothermelFireManager.update`` with ignitions between updates.

Runs only in the build container (needs the reference; see ``_refshim.py``), on the helpers of ``make_golden.py``.  The reference has
no call that ignites during an episode; the definition is an insertion into its own lists: before chosen
updates real ``Fire`` sprites of duration 0 are put into ``mgr.sprites`` / ``mgr.durations`` at the place that keeps the order every
``update()`` leaves (by age, oldest first; inside an age by (y, x), fire.py:566-587) and ``fire_map[y, x] = BURNING`` - for the
listed cells that are UNBURNED, each once.  Everything after that is the reference's own ``update()``.

A fixture holds the per-update maps (u8), status, ``elapsed_time``, the final ``burn_amounts``, the reference-evaluated R table, the
control-line schedule (update, x, y, type) and the ignition schedule (update, x, y) AS REQUESTED - rows on cells that are not
UNBURNED and repeated rows included, which a replay has to skip itself.  Usage::

    python tests/golden/make_golden_ignite.py [--selfcheck]     # --selfcheck: replay through tests/_ignite_oracle.py too
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden as mg  # noqa: E402  (installs the reference imports through _refshim)
from simfire.enums import BurnStatus, GameStatus  # noqa: E402
from simfire.game.sprites import Fire  # noqa: E402

UNBURNED, BURNING = int(BurnStatus.UNBURNED), int(BurnStatus.BURNING)


def insert_fires(mgr, fire_map, points):
    """The definition, on the real manager: returns the cells lit."""
    lit = []
    for x, y in points:
        x, y = int(x), int(y)
        if fire_map[y, x] == UNBURNED and (x, y) not in lit:
            lit.append((x, y))
    k = len(mgr.durations)
    while k > 0 and mgr.durations[k - 1] == 0:
        k -= 1
    assert all(d > 0 for d in mgr.durations[:k])
    young = list(mgr.sprites[k:]) + [Fire((x, y), mgr.fire_size, mgr.headless) for x, y in lit]
    young.sort(key=lambda s: (s.rect.y, s.rect.x))
    mgr.sprites = list(mgr.sprites[:k]) + young
    mgr.durations = list(mgr.durations[:k]) + [0] * len(young)
    for x, y in lit:
        fire_map[y, x] = BURNING
    return lit


def run_case(case, selfcheck=False):
    """``case['ignite']``: rows (update, x, y), or a function (update, mgr, fire_map) -> [(x, y)] that picks them from the state;
    the rows of update s are inserted right before update number s (0-based), behind that update's control lines."""
    H, W = case["shape"]
    mgr, lines = mg.build_reference_manager(case)
    fire_map = np.full((H, W), UNBURNED)
    x0, y0 = case["init_pos"]
    fire_map[y0, x0] = BURNING
    rt = mg.reference_rtable(case, mgr)
    orc = None
    if selfcheck:
        import _ignite_oracle
        orc = _ignite_oracle.IgniteFire((H, W), case["init_pos"], rt, case["max_fire_duration"], case["pixel_scale"], case["update_rate"],
                                        max_time=case["max_time"], attenuate_line_ros=bool(case["attenuate"]),
                                        diagonal_spread=bool(case["diagonal"]))
    sched = np.asarray(case.get("schedule", np.zeros((0, 4), dtype=np.int64)), dtype=np.int64).reshape(-1, 4)
    ign = case["ignite"]
    maps, status, elapsed, asked, n_lit = [], [], [], [], 0
    for s in range(case["n_steps"]):
        pts = sched[sched[:, 0] == s]
        for mgr_line, kind in zip(lines, (3, 4, 5)):
            fire_map = mgr_line.update(fire_map, [(int(x), int(y)) for (_, x, y, t) in pts if t == kind])
        req = ign(s, mgr, fire_map) if callable(ign) else [(int(x), int(y)) for (u, x, y) in ign if u == s]
        asked += [(s, x, y) for x, y in req]
        n_lit += len(insert_fires(mgr, fire_map, req))
        fire_map, st = mgr.update(fire_map)
        maps.append(fire_map.astype(np.uint8).copy())
        status.append(1 if st == GameStatus.RUNNING else 0)
        elapsed.append(float(mgr.elapsed_time))
        if orc is not None:
            orc.apply_mitigation([(int(x), int(y), int(t)) for (_, x, y, t) in pts])
            orc.ignite(req)
            orc.update()
            assert (orc.fire_map == fire_map).all(), f"{case['name']}: the wrapper's map differs at update {s}"
            assert (orc.fire.burn == np.array(mgr.burn_amounts, dtype=np.float64)).all(), f"{case['name']}: burn differs at update {s}"
            assert orc.fire.elapsed_time == mgr.elapsed_time and orc.running == (st == GameStatus.RUNNING)
        if st != GameStatus.RUNNING:
            break
    out = dict(shape=np.array([H, W]), init_pos=np.array(case["init_pos"]), pixel_scale=np.float64(case["pixel_scale"]),
               update_rate=np.float64(case["update_rate"]), max_fire_duration=np.int64(case["max_fire_duration"]),
               max_time=np.float64(np.nan if case["max_time"] is None else case["max_time"]), attenuate=np.int64(case["attenuate"]),
               diagonal=np.int64(case["diagonal"]), schedule=sched, ignite=np.array(asked, dtype=np.int64).reshape(-1, 3),
               fire_maps=np.stack(maps), status=np.array(status, dtype=np.int8), elapsed=np.array(elapsed),
               burn=np.array(mgr.burn_amounts, dtype=np.float64), rtable=rt, n_lit=np.int64(n_lit))
    path = os.path.join(HERE, f"ignite_{case['name']}.npz")
    np.savez_compressed(path, **out)
    print(f"  {os.path.basename(path)}: {len(status)} updates, {len(asked)} rows asked, {n_lit} cells lit, final status {status[-1]}, "
          f"{os.path.getsize(path) / 1024:.0f} KiB")


def chaparral(H, W):
    return dict(w_0=np.full((H, W), 0.9810356625846572), delta=np.full((H, W), 5.890006842991012),
                M_x=np.full((H, W), 0.9833113830744984), sigma=np.full((H, W), 3433.643783383716))


def mixed(H, W, seed):
    codes, elev, U, U_dir = mg.mixed_terrain(H, W, seed)
    w0, de, mx, sg = mg.fuel_arrays(codes)
    return dict(elevation=elev, U=U, U_dir=U_dir, w_0=w0, delta=de, M_x=mx, sigma=sg)


def beside_newest(updates, offsets):
    """Picks, before the named updates, the cells at ``offsets`` from the sprites the last update created: an ignited cell and an
    update-ignited cell of the same age then share a candidate neighbour, on either side of it in the (y, x) order."""
    def pick(s, mgr, fire_map):
        if s not in updates:
            return []
        H, W = fire_map.shape
        out = []
        for sp, d in zip(mgr.sprites, mgr.durations):
            if d == 0:
                for dx, dy in offsets:
                    x, y = sp.rect.x + dx, sp.rect.y + dy
                    if 0 <= x < W and 0 <= y < H:
                        out.append((x, y))           # (whatever the cell is: a replay skips what is not UNBURNED, and repeats)
        return out[:24]
    return pick


def all_cases():
    cases = []
    # a second start at update 0, before and behind the reset's cell in the (y, x) order, and a third one later
    H = W = 32
    cases.append(mg.base_case("second_start", H, W, init_pos=(8, 8), n_steps=24, **chaparral(H, W),
                              ignite=[(0, 22, 20), (0, 9, 3), (0, 9, 8), (0, 8, 8), (5, 26, 6), (5, 26, 6), (11, 8, 8), (11, 2, 29)]))
    # a backfire lit from a FIRELINE towards the head fire (the wind blows it east): the fronts meet; beside it, cells two away from
    # the head fire's newest sprites - the tie between an ignited cell and an update-ignited one of the same age
    H, W = 30, 40
    wall = [(0, 30, y, 3) for y in range(2, 28)]
    back = [(4, 29, y) for y in range(6, 24)] + [(4, 30, 10), (4, 29, 6)]           # (one row on the line itself, one twice)
    tie = beside_newest({2, 3, 6, 7, 9}, ((2, 0), (-2, 0), (0, 2), (0, -2), (2, 1), (-2, -1)))

    def backfire(s, mgr, fire_map):
        return [(x, y) for (u, x, y) in back if u == s] + tie(s, mgr, fire_map)
    cases.append(mg.base_case("backfire", H, W, init_pos=(10, 15), n_steps=28, U=9.0 * 88, U_dir=270.0, **chaparral(H, W),
                              schedule=np.array(wall), ignite=backfire))
    # ignitions next to lines of every type, attenuation on, mixed fuels and wind; rows on line cells, burning and burned cells
    H, W = 28, 36
    sched = [(0, 12, y, 3) for y in range(3, 25)] + [(0, x, 20, 5) for x in range(13, 34)] + [(3, 24, y, 4) for y in range(2, 19)]
    ign = [(1, 11, y) for y in (5, 6, 12)] + [(1, 13, 7), (1, 12, 8), (2, 20, 19), (2, 20, 21), (2, 20, 20), (6, 23, 5), (6, 25, 5),
                                             (6, 24, 5), (6, 18, 10), (9, 18, 10), (9, 30, 3), (14, 18, 10), (14, 2, 26)]
    cases.append(mg.base_case("beside_lines", H, W, init_pos=(18, 10), n_steps=30, max_fire_duration=5, pixel_scale=30.0, attenuate=1,
                              schedule=np.array(sched), ignite=ign, **mixed(H, W, 31)))
    # 4-connected spread, several starts at several updates and the tie picker
    tie4 = beside_newest({3, 4, 8}, ((2, 0), (0, 2), (-1, -1), (1, 1)))

    def four(s, mgr, fire_map):
        return {0: [(30, 4)], 6: [(5, 22), (6, 22), (5, 23)], 12: [(33, 25), (33, 25)]}.get(s, []) + tie4(s, mgr, fire_map)
    cases.append(mg.base_case("four_connected", H, W, init_pos=(16, 12), n_steps=30, max_fire_duration=5, pixel_scale=30.0, attenuate=0,
                              diagonal=0, ignite=four, **mixed(H, W, 47)))
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--selfcheck", action="store_true")
    a = ap.parse_args()
    for case in all_cases():
        run_case(case, selfcheck=a.selfcheck)


if __name__ == "__main__":
    main()
