"""Ensemble statistics on the GPU (``sf_ensemble_stats``).  Expected values always come from
``tests/_ensemble_oracle.py`` fed with ``eng.arrival(e)`` of the same handle - the older getter, which ``tests/test_arrival_gpu.py``
holds against the maps - never from the kernel under test.  Every output is compared for equality.  Run with ``pytest -m gpu``."""
import ctypes as C

import numpy as np
import pytest

import _ensemble_oracle as eo
import _ensemble_worlds as ew

pytestmark = pytest.mark.gpu

ALL = dict(count=True, prob=True, first=True, mean=True, loss=True)
NAMES = ("count", "prob", "first", "mean", "loss")


def _engine(case, mode, values=True):
    """(engine behind its reset with recording on and, with ``values``, the case's plane; E; the plane; ignitions)"""
    from simfire_amd.engine import FireEngine
    kw, R8, E, inits = ew.world(case)
    eng = FireEngine(n_envs=E, **kw)
    m = ew.mode_settings(mode)
    eng.set_fused(m["fused"])
    if m.get("tuning"):
        eng.set_tuning(**m["tuning"])
    eng.set_rtable(R8)
    eng.reset(inits)
    eng.enable_arrival(True)
    plane = ew.make_values(case, E, inits) if values else None
    if values:
        eng.values_set(plane)
    return eng, E, plane, inits


def _arrivals(eng, E):
    return np.stack([eng.arrival(e) for e in range(E)])


def _same(got, want, tag):
    assert set(got) == set(want), (tag, sorted(got), sorted(want))
    for n, w in want.items():
        g = got[n].cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, n, g.dtype, g.shape, w.dtype, w.shape)
        bad = np.argwhere(g != w)
        assert not len(bad), (tag, n, len(bad), bad[:5].tolist(), [(g[tuple(i)].item(), w[tuple(i)].item()) for i in bad[:5]])


def _check(eng, arr, members, horizons, plane, tag):
    want = eo.stats(arr, members, horizons, plane)
    got = eng.ensemble_stats(members, horizons=horizons, **{n: n in want for n in NAMES})
    _same(got, want, tag)
    return want


# ------------------------------------------------------------------ 1. statistics at several moments of an episode
@pytest.mark.parametrize("case,mode", ew.PAIRS, ids=["%s-%s" % p for p in ew.PAIRS])
def test_statistics_through_an_episode(case, mode):
    """Behind calls of 1, 2, 3, 5, 7, 11 updates: all five outputs of every member layout, with T = 1, 3 and 8 taking turns, equal the
    oracle's.  The case sees counts above E (the K = 67 group) and first / mean cells nobody has reached."""
    eng, E, plane, _ = _engine(case, mode)
    lay = ew.layouts(E)
    if case == "70x1030_wide":
        assert eng.geometry()["pitch"] > 1024
    top, nobody, kinds = 0, 0, []
    for moment, n in enumerate(ew.CALLS):
        eng.step(n)
        kinds.append((n, eng.last_launch_kind(), eng.cell_layout()))
        arr = _arrivals(eng, E)
        for j, (name, members) in enumerate(lay.items()):
            hz = ew.horizons_at(moment, j)
            want = _check(eng, arr, members, hz, plane, (case, mode, moment, name, hz))
            top = max(top, int(want["count"].max()))
            nobody += int((want["first"] == -1).sum())
    print("launches (n, kind, layout):", case, mode, kinds, "largest count", top)
    assert top > E and nobody > 0
    if mode.startswith("run"):
        assert all((kind, layout) == (2, 1) for _, kind, layout in kinds), kinds      # the resident launch and its blocked plane throughout


# ------------------------------------------------------------------ 2. members out of step
def test_members_out_of_step():
    """Two environments restart in the middle: one member is at update 2 while the others are at 20.  One of the two is ringed by
    fire lines and goes out: a frozen member.  The plane is taken as it stands."""
    eng, E, plane, _ = _engine(ew.SCRIPT_CASE, "run")
    o = ew.OUT_OF_STEP
    lay = ew.layouts(E)
    eng.step(o["first"])
    eng.reset_envs(list(o["reset"]), np.array(o["xy"], dtype=np.int32))
    ringed = o["ringed"]
    eng.apply_mitigation([(ringed, x, y, t) for (x, y, t) in ew.ring(*o["xy"][o["reset"].index(ringed)])])
    for i, n in enumerate(o["then"]):
        eng.step(n)
        st, _ = eng.status()
        if i == 0:
            assert st[:, 1].tolist() == [2 if e in o["reset"] else 20 for e in range(E)]
        else:
            assert st[ringed, 0] != 1 and st[ringed, 1] < st[o["reset"][0], 1]
        arr = _arrivals(eng, E)
        for name in ("all", "g3k5", "k7"):
            _check(eng, arr, lay[name], (0, 2, 5, ew.MID, 20, -1), plane, ("out of step", i, name))
    assert (arr[ringed] >= 0).sum() == 1


# ------------------------------------------------------------------ 3. loss
@pytest.mark.parametrize("case,mode", [("24x40", "run"), ("33x17", "fused0")])
def test_loss(case, mode):
    """A shared (24x40) and a per-environment (33x17) plane with negative values: ``loss`` equals the oracle's; with horizon -1
    and a duplicate-free group it equals the sum of ``damage()`` over the members."""
    eng, E, plane, _ = _engine(case, mode)
    assert (plane < 0).any() and plane.ndim == (3 if case == "33x17" else 2)
    lay = ew.layouts(E)
    eng.step(7)
    eng.step(4)
    arr = _arrivals(eng, E)
    for name, members in lay.items():
        want = _check(eng, arr, members, (0, 3, 6, -1), plane, (case, "loss", name))
        assert (want["loss"][:, -1] != 0).any()
    dmg = eng.damage()
    for members in (lay["all"], lay["k1"], np.array([[E - 1, 0], [1, 2]], dtype=np.int32)):
        got = eng.ensemble_stats(members, horizons=(-1,), prob=False, loss=True)["loss"].cpu().numpy()
        assert got.shape == (members.shape[0], 1) and (got[:, 0] == dmg[members].sum(axis=1)).all(), (got.tolist(), dmg.tolist())
    hit = np.broadcast_to(plane, arr.shape)[arr >= 0]
    assert (hit < 0).any() and (hit > 0).any()                    # negative values were reached and counted


def test_loss_needs_a_plane():
    from simfire_amd import _lib
    eng, E, _, _ = _engine("24x40", "fused0", values=False)
    eng.step(6)
    with pytest.raises(_lib.SimfireHipError, match="sf_values_set"):
        eng.ensemble_stats(None, loss=True)
    arr = _arrivals(eng, E)
    _check(eng, arr, ew.layouts(E)["g3k5"], (2, -1), None, "no plane")


# ------------------------------------------------------------------ 4. only what is asked for
@pytest.mark.parametrize("case", ["24x40", "33x17"])
def test_only_what_is_asked_for(case):
    import torch
    from simfire_amd import _lib
    eng, E, plane, _ = _engine(case, "run")
    eng.step(9)
    members = ew.layouts(E)["g3k5"]
    hz = (1, 5, -1)
    every = eng.ensemble_stats(members, horizons=hz, **ALL)
    for n in NAMES:
        one = eng.ensemble_stats(members, horizons=hz, **{k: k == n for k in NAMES})
        assert list(one) == [n] and torch.equal(one[n], every[n]), n
    # the raw ABI with outputs that are slices of larger tensors: the guard elements in front and behind stay; shift 16 keeps the
    # slices 16-byte aligned (quad stores where W % 4 == 0), shift 1 does not (dword stores)
    G, K, T = members.shape[0], members.shape[1], len(hz)
    p = _lib.SfEnsembleParams(n_groups=G, group_size=K, n_horizons=T)
    for t, h in enumerate(hz):
        p.horizons[t] = h
    for shift in (16, 1):
        big, ptrs = {}, {}
        for n in NAMES:
            ref = every[n]
            fill = -7 if ref.dtype != torch.float32 else -7.5
            big[n] = torch.full((ref.numel() + 2 * shift,), fill, dtype=ref.dtype, device=ref.device)
            ptrs[n] = big[n][shift:].data_ptr()
        torch.cuda.synchronize()
        o = _lib.SfEnsembleOut(**ptrs)
        assert eng._L.sf_ensemble_stats(eng._h, C.byref(p), members.ctypes.data_as(C.c_void_p), C.byref(o)) == _lib.SF_OK
        eng.sync()
        for n in NAMES:
            ref = every[n]
            assert torch.equal(big[n][shift:shift + ref.numel()], ref.reshape(-1)), (shift, n)
            guard = torch.cat([big[n][:shift], big[n][shift + ref.numel():]])
            assert (guard == (-7 if ref.dtype != torch.float32 else -7.5)).all(), (shift, n)


# ------------------------------------------------------------------ 5. the call changes nothing
@pytest.mark.parametrize("mode", ["run", "fused0"])
def test_the_call_changes_nothing(mode):
    import torch
    eng, E, plane, _ = _engine("24x40", mode)
    eng.step(5)
    eng.step(3)
    members = ew.layouts(E)["g3k5"]
    hz = (0, 4, -1)
    before = (eng.last_launch_kind(), eng.cell_layout(), eng.damage().tolist(), [a.tolist() for a in eng.status()])
    a = eng.ensemble_stats(members, horizons=hz, **ALL)
    b = eng.ensemble_stats(members, horizons=hz, **ALL)
    after = (eng.last_launch_kind(), eng.cell_layout(), eng.damage().tolist(), [a_.tolist() for a_ in eng.status()])
    assert before == after
    for n in NAMES:
        assert a[n].cpu().numpy().tobytes() == b[n].cpu().numpy().tobytes(), n
    blob0 = eng.save_state(list(range(E))).tobytes()
    layout = eng.cell_layout()
    c = eng.ensemble_stats(members, horizons=hz, **ALL)
    assert eng.cell_layout() == layout and eng.save_state(list(range(E))).tobytes() == blob0
    eng.set_async(True)
    d = eng.ensemble_stats(members, horizons=hz, **ALL)
    eng.sync()
    eng.set_async(False)
    for n in NAMES:
        assert torch.equal(c[n], a[n]) and torch.equal(d[n], a[n]), n
    eng.step(4)                                                   # and the handle goes on
    _check(eng, _arrivals(eng, E), members, hz, plane, "afterwards")


# ------------------------------------------------------------------ 6. the counterfactual recipe
@pytest.mark.parametrize("mode", ["run", "fused0"])
def test_counterfactual_recipe(mode):
    """Environment 0 forked into all others after a few updates, control lines of its own for every member through
    ``step_mitigated``, several calls: the statistics equal the oracle's and the burn probability is not 0 / 1 everywhere."""
    eng, E, plane, inits = _engine(ew.SCRIPT_CASE, mode)
    eng.step(4)
    eng.copy_envs([0] * (E - 1), list(range(1, E)))
    lay = ew.layouts(E)
    for i, pts in enumerate(ew.recipe_points(E, inits)):
        eng.step_mitigated(pts)
        arr = _arrivals(eng, E)
        for name in ("all", "k6", "k67"):
            want = _check(eng, arr, lay[name], (4, 6, 9, -1), plane, ("recipe", i, name))
    p = eng.ensemble_stats(None, horizons=(6, -1))["prob"].cpu().numpy()
    assert ((p > 0) & (p < 1)).sum() >= 20, np.unique(p).tolist()
    assert (want["count"][0, 0] == 67 * (arr[0] >= 0) * (arr[0] <= 4)).all()      # up to the fork the members are one fire


def test_simulation_class_burn_probability():
    """``BatchedFireSimulation.burn_probability`` / ``ensemble_stats``: complete on return, as NumPy or as a tensor."""
    import os
    import torch
    import yaml
    from simfire_amd.config import Config
    from simfire_amd.simulation import BatchedFireSimulation
    from test_env_state_gpu import CFG
    y = yaml.safe_load(open(os.path.join(CFG, "functional_config.yml")))
    y["area"]["screen_size"] = [96, 96]
    y["terrain"]["topography"]["functional"]["function"] = "flat"
    y["simulation"]["headless"] = True
    bat = BatchedFireSimulation(Config(config_dict=y), 4, ignitions=[(40, 40), (44, 42), (48, 50), (52, 44)])
    bat.enable_arrival(True)
    bat.run(9, return_maps=False)
    arr = bat.arrival()
    members = [[0, 1, 2, 3], [3, 3, 1, 0]]
    want = eo.stats(arr, members, (3, 6, -1))
    p = bat.burn_probability(members, horizons=(3, 6, -1))
    assert isinstance(p, np.ndarray) and p.dtype == np.float32 and (p == want["prob"]).all() and ((p > 0) & (p < 1)).any()
    now = bat.burn_probability(device=True)
    assert isinstance(now, torch.Tensor) and now.is_cuda and tuple(now.shape) == (1, 96, 96)
    assert (now.cpu().numpy() == eo.stats(arr, [[0, 1, 2, 3]], (-1,))["prob"][:, 0]).all()
    got = bat.ensemble_stats(members, horizons=(3, 6, -1), count=True, first=True, mean=True)
    _same(got, {k: want[k] for k in ("count", "prob", "first", "mean")}, "BatchedFireSimulation")


# ------------------------------------------------------------------ 7. against the torch assembly
def test_against_the_torch_assembly():
    import torch
    eng, E, _, _ = _engine("72x80_win", "run_win", values=False)
    eng.step(11)
    eng.step(7)
    members = ew.layouts(E)["g3k5"]
    hz = (0, 6, ew.MID, -1)
    got = eng.ensemble_stats(members, horizons=hz, count=True, prob=False, first=True)
    count, first = eo.torch_assembly(eng.arrival_torch(), members, hz)
    assert count.device == got["count"].device
    assert torch.equal(got["count"], count) and torch.equal(got["first"], first.to(torch.int32))
    assert int(count.max()) >= 3


# ------------------------------------------------------------------ 8. refusals
def test_refusals():
    import torch
    from simfire_amd import _lib
    from simfire_amd.engine import FireEngine
    kw, R8, E, inits = ew.world("24x40")
    eng = FireEngine(n_envs=E, **kw)
    eng.set_fused(0)
    eng.set_rtable(R8)
    eng.reset(inits)
    eng.step(3)
    H, W = kw["shape"]
    bufs = {n: torch.zeros(2 * 8 * H * W + 8, dtype=torch.int64, device="cuda") for n in NAMES}

    def raw(members=((0, 1), (2, 2)), hz=(0, -1), G=None, K=None, T=None, reserved=0, outs=NAMES, null=()):
        m = np.ascontiguousarray(members, dtype=np.int32)
        p = _lib.SfEnsembleParams(n_groups=m.shape[0] if G is None else G, group_size=m.shape[1] if K is None else K,
                                  n_horizons=len(hz) if T is None else T, reserved=reserved)
        for t, h in enumerate(hz[:8]):
            p.horizons[t] = h
        o = _lib.SfEnsembleOut(**{n: (bufs[n].data_ptr() + outs[n] if isinstance(outs, dict) else bufs[n].data_ptr()) for n in outs})
        return eng._L.sf_ensemble_stats(None if "sim" in null else eng._h, None if "params" in null else C.byref(p),
                                        None if "members" in null else m.ctypes.data_as(C.c_void_p), None if "out" in null else C.byref(o))

    assert raw(outs=("count",)) == _lib.SF_ESTATE                 # before enable_arrival
    with pytest.raises(_lib.SimfireHipError, match="sf_enable_arrival"):
        eng.ensemble_stats(None)
    eng.enable_arrival(True)
    assert raw(outs=("count", "prob", "first", "mean")) == _lib.SF_OK
    assert raw() == _lib.SF_ESTATE                                # loss without a value plane
    eng.values_set(ew.make_values("24x40", E, inits))
    assert raw() == _lib.SF_OK
    for null in ("sim", "params", "members", "out"):
        assert raw(null=(null,)) == _lib.SF_EINVAL, null
    big = 1 << 20
    for name, kwargs in {
        "no output": dict(outs=()),
        "G = 0": dict(G=0), "K = 0": dict(K=0), "K = 65536": dict(K=65536), "G negative": dict(G=-1),
        "G * K beyond 2^20": dict(G=big // 2 + 1, K=2), "T = 0": dict(T=0), "T = 9": dict(hz=tuple(range(9)), T=9),
        "descending": dict(hz=(5, 3)), "equal": dict(hz=(3, 3)), "below -1": dict(hz=(-2,)), "-1 not last": dict(hz=(-1, 4)),
        "-1 in the middle": dict(hz=(0, -1, 4)), "reserved": dict(reserved=1),
        "member E": dict(members=((0, E), (1, 1))), "member -1": dict(members=((0, 1), (-1, 1))),
        "misaligned count": dict(outs={"count": 2}), "misaligned loss": dict(outs={"loss": 4}),
    }.items():
        assert raw(**kwargs) == _lib.SF_EINVAL, name
        assert b"sf_ensemble_stats" in eng._L.sf_last_error()
    # the handle works afterwards
    eng.step(5)
    arr = _arrivals(eng, E)
    _check(eng, arr, ew.layouts(E)["g3k5"], (0, 4, -1), ew.make_values("24x40", E, inits), "after the refusals")
