"""The per-environment oracle (tests/_per_env_oracle.py) that the per-environment terrain tests compare the device with: with one
table for every environment it equals ``DenseOracle(n_envs=E)``; with a table per environment each environment equals a run of its
own; a replayed fork equals the run it copies.  No GPU needed."""
import numpy as np

from _per_env_oracle import PerEnvOracle
from oracle import fire_dense


def _kw(H, W, att, max_time=None):
    return dict(shape=(H, W), max_fire_duration=3, pixel_scale=20.0, update_rate=1.0, max_time=max_time,
                attenuate_line_ros=att, diagonal_spread=True)


def _table(rng, H, W, scale=1.0):
    R8 = rng.choice([0.0, 3.0, 7.5, 12.0, 30.0, 400.0], size=(8, H, W)) * scale
    R8[:, rng.random((H, W)) < 0.1] = 0.0
    return R8


def _drive(rng, oracles, E, H, W, calls=12):
    """The same random calls on every oracle in `oracles`."""
    for t in range(calls):
        if t % 3 == 1:
            pts = [(int(rng.integers(E)), int(rng.integers(W)), int(rng.integers(H)), int(rng.integers(3, 6))) for _ in range(10)]
            for o in oracles:
                o.apply_mitigation(pts)
        if t == 7:
            e0, x, y = int(rng.integers(E)), int(rng.integers(W)), int(rng.integers(H))
            for o in oracles:
                o.reset_env(e0, x, y)
        if t == 9:
            m = oracles[0].fire_map(1).copy()
            m[rng.random((H, W)) < 0.05] = 0
            for o in oracles:
                o.load_fire_map(1, m)
        n = int(rng.integers(1, 6))
        for o in oracles:
            o.step(n)


def test_one_table_for_all_equals_the_multi_environment_oracle():
    rng = np.random.default_rng(1)
    H, W, E = 30, 41, 4
    for att in (False, True):
        kw = _kw(H, W, att, max_time=25.0)
        R8 = _table(rng, H, W)
        per = PerEnvOracle(n_envs=E, **kw)
        multi = fire_dense.DenseOracle(n_envs=E, **kw)
        inits = [(int(rng.integers(W)), int(rng.integers(H))) for _ in range(E)]
        for o in (per, multi):
            o.set_rtable(R8)
            o.reset(inits)
        _drive(rng, (per, multi), E, H, W)
        st, el = per.status()
        so, eo = multi.status()
        assert st.shape == (E, 8) and (st == so).all() and (el == eo).all()
        assert st[:, 4].sum() > 0                                 # (something burned)
        for e in range(E):
            assert (per.fire_map(e) == multi.fire_map(e)).all(), e
            assert (per.burn(e) == multi.burn(e)).all(), e
            assert (per.parents(e) == multi.parents(e)).all(), e


def test_a_table_per_environment_equals_separate_runs():
    rng = np.random.default_rng(2)
    H, W, E = 33, 47, 3
    kw = _kw(H, W, True)
    tabs = [_table(rng, H, W, 1 + e) for e in range(E)]
    per = PerEnvOracle(n_envs=E, **kw)
    solo = [fire_dense.DenseOracle(n_envs=1, **kw) for _ in range(E)]
    for e in range(E):
        per.set_rtable(tabs[e], env=e)
        solo[e].set_rtable(tabs[e])
        assert (per.get_rtable(e) == tabs[e]).all()
    inits = [(int(rng.integers(W)), int(rng.integers(H))) for _ in range(E)]
    per.reset(inits)
    for e in range(E):
        solo[e].reset([inits[e]])
    for t in range(10):
        pts = [(e, int(rng.integers(W)), int(rng.integers(H)), 3 + t % 3) for e in range(E)]
        per.apply_mitigation(pts)
        for (e, x, y, ty) in pts:
            solo[e].apply_mitigation([(0, x, y, ty)])
        per.step(2)
        for o in solo:
            o.step(2)
    st, el = per.status()
    for e in range(E):
        so, eo = solo[e].status()
        assert (st[e] == so[0]).all() and el[e] == eo[0], e
        assert (per.fire_map(e) == solo[e].fire_map(0)).all(), e
        assert (per.burn(e) == solo[e].burn(0)).all(), e
    # the tables do tell the environments apart: the same history over environment 0's table ends elsewhere
    other = fire_dense.DenseOracle(n_envs=1, **kw)
    other.set_rtable(tabs[0])
    other.reset([inits[1]])
    other.step(20)
    assert not (other.burn(0) == per.burn(1)).all()


def test_a_replayed_fork_equals_the_run_it_copies():
    """copy_env: with terrain the copy goes on over the source's table, without over its own; a table changed in the source's
    history is replayed as it was; a source in another oracle (a state loaded into another handle)."""
    rng = np.random.default_rng(3)
    H, W, E = 28, 36, 3
    kw = _kw(H, W, False)
    tabs = [_table(rng, H, W, 1 + e) for e in range(E + 1)]
    per = PerEnvOracle(n_envs=E, **kw)
    for e in range(E):
        per.set_rtable(tabs[e], env=e)
    per.reset([(5, 5), (20, 10), (30, 25)])
    per.step(4)
    per.set_rtable(tabs[E], env=0)                               # a new table in the middle of environment 0's history
    per.apply_mitigation([(0, 6, 6, 4)])
    per.step(3)
    refs = {}
    for terrain, dst in ((True, 1), (False, 2)):
        ref = fire_dense.DenseOracle(n_envs=1, **kw)
        ref.set_rtable(tabs[0])
        ref.reset([(5, 5)])
        ref.step(4)
        ref.set_rtable(tabs[E])
        ref.apply_mitigation([(0, 6, 6, 4)])
        ref.step(3)
        ref.set_rtable(tabs[E] if terrain else tabs[dst])
        per.copy_env(0, dst, terrain=terrain)
        assert (per.get_rtable(dst) == (tabs[E] if terrain else tabs[dst])).all()
        refs[dst] = ref
    per.step(5)
    for dst, ref in refs.items():
        ref.step(5)
        assert (per.fire_map(dst) == ref.fire_map(0)).all() and (per.burn(dst) == ref.burn(0)).all(), dst
        assert (per.status()[0][dst] == ref.status()[0][0]).all()
    assert not (per.burn(1) == per.burn(2)).all()                 # (the tables made a difference)
    recv = PerEnvOracle(n_envs=2, **kw)
    recv.set_rtable(tabs[1], env=1)
    recv.copy_env(2, 1, source=per)
    assert (recv.get_rtable(1) == tabs[1]).all()
    assert (recv.fire_map(1) == per.fire_map(2)).all() and (recv.status()[0][1] == per.status()[0][2]).all()
