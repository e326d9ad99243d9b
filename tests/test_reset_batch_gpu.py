"""Resets on the GPU (``sf_reset`` / ``sf_reset_env`` / ``sf_reset_envs`` / ``sf_reset_where``): every entry runs
the same two kernels, so a twin handle alone pins nothing.  The yardsticks are the recorded parent - SHA-256 digests of the twin
worlds of section 1 (``PARENT`` below), taken on the library of the last commit that still had the separate ``sf_reset_env`` path
(memsets + ``k_init_env`` + ``k_rebuild_seams``), on its ``sf_reset_env`` twin - and ``oracle/fire_dense.c`` replaying every
environment's log from its last reset.  ``python tests/test_reset_batch_gpu.py`` prints the table of twin A (how ``PARENT`` was
recorded, with ``SIMFIRE_HIP_LIB`` naming that commit's library).  Run with ``pytest -m gpu``."""
import hashlib

import numpy as np
import pytest

from oracle import fire_dense
from test_env_state_gpu import MODES, RESIDENT, _Replay, _check, _world

pytestmark = pytest.mark.gpu


def _make(kw, E, mode, R8, inits, prune=False, graph=False, per_env=False):
    from simfire_amd.engine import FireEngine
    eng = FireEngine(n_envs=E, per_env_terrain=per_env, **kw)
    m = MODES[mode]
    eng.set_fused(m["fused"])
    if m.get("tuning"):
        eng.set_tuning(**m["tuning"])
    if prune:
        eng.set_prune_after_quit(True)
    if graph:
        eng.enable_spread_graph(True)
    if per_env:
        for e in range(E):
            eng.set_rtable(R8[e], env=e)
    else:
        eng.set_rtable(R8)
    eng.reset(inits)
    return eng


def _blobs(eng):
    return eng.save_state(list(range(eng.n_envs)))


def _same(a, b, tag):
    ba, bb = _blobs(a), _blobs(b)
    for e in range(a.n_envs):
        assert ba[e].tobytes() == bb[e].tobytes(), (tag, "state blob of environment", e)
    sa, ea = a.status()
    sb, eb = b.status()
    assert (sa == sb).all() and ea.tobytes() == eb.tobytes(), (tag, sa, sb)
    return bb


def _digest(eng, maps=False):
    """SHA-256 of the concatenated state blobs; with ``maps`` also of ``fire_maps()`` and every ``burn(e)`` behind them."""
    h = hashlib.sha256(_blobs(eng).tobytes())
    if maps:
        h.update(eng.fire_maps().tobytes())
        for e in range(eng.n_envs):
            h.update(eng.burn(e).tobytes())
    return h.hexdigest()


def _points(rng, E, H, W, p=0.35):
    pts = []
    for e in range(E):
        if rng.random() < p:
            pts += [(e, int(rng.integers(W)), int(rng.integers(H)), int(rng.integers(3, 6))) for _ in range(int(rng.integers(1, 5)))]
    return pts


# ------------------------------------------------------------------ 1. equal to the sf_reset_env loop
def _twin_world(seed, mode, H, W, md, att, prune=False, graph=False, E=None, before=(4, 14), after=(10, 31)):
    """Handles A and B built alike and driven through the same random log; at a random update a random subset is reset - A with the
    ``sf_reset_env`` loop, B with one ``sf_reset_envs``.  All state blobs and the result block equal then and after 10 - 30 further
    updates; on B the blobs of the environments that were not reset are what they were before the call.  Returns the digests of
    A and of B: (straight after the reset, at the end)."""
    rng = np.random.default_rng(seed)
    E = int(rng.integers(4, 9)) if E is None else E
    kw, R8 = _world(rng, H, W, md, att, diag=True)
    inits = [(int(rng.integers(W)), int(rng.integers(H))) for _ in range(E)]
    a, b = (_make(kw, E, mode, R8, inits, prune, graph) for _ in range(2))
    resident = mode in RESIDENT and md <= 5 and not graph
    chunk = 1 if mode in ("fused0", "fused1") else int(rng.integers(2, 4))

    def drive(n_updates):
        t = 0
        while t < n_updates:
            pts = _points(rng, E, H, W)
            n = min(chunk, n_updates - t)
            for x in (a, b):
                if pts:
                    x.apply_mitigation(pts)
                x.step(n)
            t += n

    drive(int(rng.integers(*before)))
    _same(a, b, (seed, mode, "before the reset"))            # (save_state / status read the plane that is current: no conversion)
    layout = b.cell_layout()
    assert a.cell_layout() == layout
    if mode != "run_kwin":                                   # (the automatic choice may step a small grid with the per-step kernels)
        assert layout == (1 if resident else 0), (mode, layout)
    was = _blobs(b)
    envs = rng.choice(E, size=int(rng.integers(1, E)), replace=False).astype(np.int32)
    xy = np.stack([rng.integers(0, W, len(envs)), rng.integers(0, H, len(envs))], axis=1).astype(np.int32)
    for e, (x, y) in zip(envs, xy):
        a.reset_env(int(e), int(x), int(y))
    b.reset_envs(envs, xy)
    assert b.cell_layout() == layout and a.cell_layout() == layout
    now = _same(a, b, (seed, mode, "after the reset", envs.tolist()))
    for e in range(E):
        if e not in envs:
            assert now[e].tobytes() == was[e].tobytes(), (seed, mode, "environment not reset changed", e)
    after_reset = [_digest(x) for x in (a, b)]
    drive(int(rng.integers(*after)))
    _same(a, b, (seed, mode, "at the end"))
    assert a.fire_maps().tobytes() == b.fire_maps().tobytes()
    for e in range(E):
        assert a.burn(e).tobytes() == b.burn(e).tobytes(), (seed, mode, e)
        if graph:
            assert (a.spread_parents(e) == b.spread_parents(e)).all()
    assert b.status()[0][:, 1].max() > 0
    return [(d, _digest(x, maps=True)) for d, x in zip(after_reset, (a, b))]


CASES = {
    "37x101_md4_att": dict(H=37, W=101, md=4, att=True),
    "64x64_md7": dict(H=64, W=64, md=7, att=False),
    "225x225_md4_prune": dict(H=225, W=225, md=4, att=False, prune=True),
    "225x225_md4_att_graph": dict(H=225, W=225, md=4, att=True, graph=True),
    "225x225_md4_att": dict(H=225, W=225, md=4, att=True),
}


CASE_1024 = dict(H=1024, W=1024, md=4, att=True, E=4, before=(20, 30), after=(10, 20))
MODES_1024 = ["run", "fused1"]

# (case, mode) -> twin A's digests (after the reset, at the end) on the parent's library: see the module docstring
PARENT = {
    ('37x101_md4_att', 'fused0'): ('5bf4c91e3f3941c3b6e4948c276d388d61fdf0bcd239a7c6428ca1f62f158f60',
                                   'f3087d5473a57a1eebe5924e45a5b1f4c3705b89504eda099b6ae304f14ce88f'),
    ('37x101_md4_att', 'fused1'): ('a9d7e1041e2fba4e2a555ec7463964959bfbe45669025b9e3f953c8647fec3b7',
                                   '1ea9dbba1642d8f56215c253fc84e79b6fbc10e5813a1806987a8df8498314ec'),
    ('37x101_md4_att', 'run'): ('9881e0f3f151ad46f1fc2e00e5334413fd7f99fbfb96cd5aadac8096278d58e6',
                                'e1ac8f471ae3ed9bb86eadb80769d10bc0b840b908494bd23db8e9c61e436de3'),
    ('37x101_md4_att', 'run_win'): ('cbd0b092cae8cbd093ba65b4ae226a6bf0b609147eb519f9ed313304fd09e0f0',
                                    '7082f2bdb9fa206ab9b37df321c89441ab98b8586baf6e9ff700eb7d41efec33'),
    ('37x101_md4_att', 'run_team'): ('201cced2ab5e2bcdd48b8f8497dc108d9b0e8c1690fadeb9b9e11fddb46b827f',
                                     '65f5ede5c2c1c359d24163291dd5960454a954cc82b2ff5d2408ff349eda0737'),
    ('37x101_md4_att', 'run_kwin'): ('c1c71fa6ce8edc252b8f91e81d5a296fa136e3dca61ece5723f11792c5ef486d',
                                     '84e422cf11b92b8316941a78ece4f34ded64d7b35016bee8b2a99d258f677c0b'),
    ('64x64_md7', 'fused0'): ('85e3bbe6a1eca4fa7845e7c787409704620170a257b407aca09b9b12c399a965',
                              '916fdaa6e760538b5b9c7fea0f632255067acfdebf6d9547fba97d4feeb862d9'),
    ('64x64_md7', 'fused1'): ('babce581b1d901471b1e205898f9d28cb6fc8ecc5c26dd9c821f7456eeb770ff',
                              '4234779b9e80ff757b4f830593ede7552e67a47265939aec407062bd191d848d'),
    ('64x64_md7', 'run'): ('596fc36eeb3fb3bd51b5c82ec61adcec58aebe95ae53143d47da015a96b8edb3',
                           'd22cd214179d7bf1e84f2f162aa8f56d52c5f82f90005782cfb5436dd41f5868'),
    ('64x64_md7', 'run_win'): ('bacb9eb84729ca0ef42b99aa56e67147184cda30076408baa11767f38a76646f',
                               '30b3877ea8dd87707f1fb2eb3ffbf17879456884818efc9ac4881ce8279770f8'),
    ('64x64_md7', 'run_team'): ('26b52f17aaf7d15dd954517240e1b0570818ddd437f7af5a24efd5c9c98e384a',
                                '68553e5980871717046e8afac04b3ea474ed5c6a96ab6d2cb9bc7684cbedd57c'),
    ('64x64_md7', 'run_kwin'): ('8dc4e9d36cca07b8203eac09f8809886687d98d9b0da5b97cb1c7b51e3d71acb',
                                'aebb2b32cde2f8aeac42e35ec5353bd1a75cd397608a696e6e91d3572b9edbca'),
    ('225x225_md4_prune', 'fused0'): ('050acb85b7002a3aadebb18f2344f0093b252ca4fb125a5dccad3b26f6c3a509',
                                      'a0f81ce709b4cee60ec1e9b926db45731dc516dd64352d48362f48e4015c5bdb'),
    ('225x225_md4_prune', 'fused1'): ('28a38e21b8a95876bff39d9b42690408955a204e2c0cc927279293ed856a8180',
                                      'aceb4d1c020c0074226a599d3c34b62d276993572f71e1537c69b590203f3bc5'),
    ('225x225_md4_prune', 'run'): ('f1857320c20bb57df50278902937155eed6a410b0c3219325e432e4851136a9f',
                                   '44ad8118cf9dff8ab14405f8730272b139ba586837fb7434e8bd9cdada65fb4b'),
    ('225x225_md4_prune', 'run_win'): ('9b4d09d5dc1d1d22b70e3c455abb02e4203e6814a780f0a04530d36b0b3fba2d',
                                       'dd7e9bbc5518022943d470669357c3cf3871eedbfcd1e7f089ebbd0474847861'),
    ('225x225_md4_prune', 'run_team'): ('88eff1de167dc17d14852534920ddc32182b8bb3a8a13add5439bff4ba2ea5d0',
                                        'e2c8a9bb54b4741c37215874f740d673575d8a2d7e98f218a3a299298bf4943b'),
    ('225x225_md4_prune', 'run_kwin'): ('16ee45d45bc225763440e9d1827c9c200c1115c53ba47ebf42982ec49a39a652',
                                        'f3fadb83d89e76ef5915e7654b9f3e97190cd43b69664083f3e8de82244819fe'),
    ('225x225_md4_att_graph', 'fused0'): ('df63f2b0079d82ea9db417a5141a3d38df430d817010ef7ef3ed9375d672923c',
                                          'bf4792c960622911a9b3bc4dd3e68269aae0d0b82f9d0353187e50357c047304'),
    ('225x225_md4_att_graph', 'fused1'): ('8d8f8746f293e86964cf03bb994686b40b1eebb5cb93914992de2fa5a37fdb00',
                                          '60cae1b285b6c076cc15ea468796af47daaedf977081a9548ebc13dd16f3aa3d'),
    ('225x225_md4_att_graph', 'run'): ('760feb4987b4dddf2cbb252c9035f9a3de13d3c23c2304f7ce3b38fe0779130f',
                                       '5b7c8d777e8fefe33c415e07999d11ca3c7b38372db4daa62932878cd8365c07'),
    ('225x225_md4_att_graph', 'run_win'): ('ac85b570b19338fca85ee389cec7ee0b7aa74622c5c1c7f4867d4ea1dac68c10',
                                           '14c8a8a4dceabbc3fdadf7ea9425ca9a9fc87c94efaf4aa59229f0d6bb505832'),
    ('225x225_md4_att_graph', 'run_team'): ('a2eacee1ba1116018f64b1a59e43778c8d4d381d617a66b60f7be9f1188022c8',
                                            '48f1d2d7ccfae164890c886a822798fd0770d16d46e5104d30936edd1e8ffb4e'),
    ('225x225_md4_att_graph', 'run_kwin'): ('49e3d910681677b2ea6895f28bc9d53d15888f692871c9da55a65c1695f447fc',
                                            '726ea9cd7b8ede6b4e1b52dc33e767e4fe24ce05b2cf523f0f6f7d95392533db'),
    ('225x225_md4_att', 'fused0'): ('60ea9c80c2875f87c74c5b4d2c2921ea8c984093edb9740b07288fa29685e89d',
                                    '5191432538a31e8fc39567e3098f94a54fe0f5a6bc9ba5afddf0fc9210c074a7'),
    ('225x225_md4_att', 'fused1'): ('089b126781890824c7828ba570659b7de3207fad6e72584dcabdda460bd9d63b',
                                    '8a5c86fd3862649fbf774045ddaea2d39dd075debdcc1cb4c86a007545d9fec0'),
    ('225x225_md4_att', 'run'): ('fb16f4d3f5a7ea1fe2e203b80978b4e3eccc3d9e30dd8db177e6c2c70f9c9378',
                                 '5c6dcbe3c0f79801bc5b3f1e32dec9a7294a6d1eb1e11a1cdedce9744f7f7009'),
    ('225x225_md4_att', 'run_win'): ('78caed4c99efc6028a0ddf9f55a89e4a6e1848c48184d30a3e3e83b4942567c8',
                                     'e2c53e2838fd882e438dbd8e73e076e71c69648881c060707c39977d1b34371d'),
    ('225x225_md4_att', 'run_team'): ('d4c823096fdf0064c6ba02649b02a3e237c9ee08829c51ed1c36bdfa5367728b',
                                      '02f5b75b1dd56e4d7e38f43beefd98827e19dd8f14ff7510147c8488909dff5a'),
    ('225x225_md4_att', 'run_kwin'): ('7d6c5c73be76f42cd6e6d778c63a5948fccf6b66db091fe93c66043932b77f1d',
                                      '2e97d1aa87b9a88252dec3568b84505c729979a83adf367c3dc8afdd477ee8b4'),
    ('1024', 'run'): ('73af9fdc38fd264293cf27164e7025d325149ba24502d56fbff722f7b1bc1b00',
                      '0309631460d7e81105c59db9c9565b546c7f509dc9f365dea33154d28d3eaa38'),
    ('1024', 'fused1'): ('39ac3a61806b37ee93e8099b63356d6b124dbf594f7eef24b465bc00dfcb6704',
                         '3698fbd5b3e82884ec87cacf791be5373156c9113a47827e9e0db47b8d9a0ff1'),
}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", list(CASES))
def test_equal_to_the_reset_env_loop(case, mode):
    da, db = _twin_world(81000 + 17 * list(CASES).index(case) + list(MODES).index(mode), mode, **CASES[case])
    print(case, mode, da, db)
    assert da == PARENT[case, mode] and db == PARENT[case, mode], (case, mode)


@pytest.mark.parametrize("mode", MODES_1024)
def test_equal_to_the_reset_env_loop_1024(mode):
    da, db = _twin_world(82000 + len(mode), mode, **CASE_1024)
    print("1024", mode, da, db)
    assert da == PARENT["1024", mode] and db == PARENT["1024", mode], mode


# ------------------------------------------------------------------ 2. equal to the oracle
@pytest.mark.parametrize("mode", list(MODES))
def test_equal_to_the_oracle(mode):
    """Every environment's log restarts at its reset; after every update fire_map, burn, result row and elapsed_time equal the
    oracle replaying the log.  Resets follow the launch the mode names directly (its plane is the current one)."""
    rng = np.random.default_rng(83000 + list(MODES).index(mode))
    H, W = (150, 165) if mode in ("run_team", "run_win", "run_kwin") else (61, 83)
    E, md = 6, 4
    kw, R8 = _world(rng, H, W, md, True, diag=True)
    kw.update(max_time=5.0, update_rate=1.0, pixel_scale=20.0)      # every episode QUITs on the runtime check at its 7th update
    R8[:] = np.maximum(R8, 30.0)                                    # (a burning cell passes its fire on in one update: no fire dies before)
    inits = [(int(rng.integers(W)), int(rng.integers(H))) for _ in range(E)]
    eng = _make(kw, E, mode, R8, inits)
    rep = _Replay(kw, False, False)
    logs = [[("table", 0), ("reset", inits[e])] for e in range(E)]
    refs = {e: rep.run(logs[e], [R8]) for e in range(E)}
    resident = mode in RESIDENT
    chunk = 1 if not resident else 2
    x0, x15 = 16 * int(rng.integers(1, W // 16)), 16 * int(rng.integers(1, W // 16)) + 15
    # update -> list of reset_envs calls (environments, ignitions)
    events = {
        4: [([0, 1, 0], [(5, 5), (W - 1, H - 1), (x0, int(rng.integers(H)))])],                 # still burning; 0 is named twice: its last ignition wins
        12: [([2, 3], [(0, 0), (x15, int(rng.integers(H)))]),                                  # after QUIT; a grid corner
             ([3], [(int(rng.integers(W)), int(rng.integers(H)))])],                           # twice in a row
        16: [([4, 5, 1], [(0, H - 1), (W - 1, 0), (x0 + 15, 0)])],
    }
    running_at = {4: [0, 1], 12: [], 16: []}
    quit_at = {4: [], 12: [2, 3], 16: [4, 5]}
    t, steps = 0, 26
    while t < steps:
        pts = _points(rng, E, H, W)
        for (e, x, y, ty) in pts:
            logs[e].append(("mit", [(x, y, ty)]))
            rep.apply(refs[e], ("mit", [(x, y, ty)]), [R8])
        if pts:
            eng.apply_mitigation(pts)
        n = min(chunk, steps - t)
        eng.step(n)
        t += n
        for e in range(E):
            logs[e] += [("step",)] * n
            for _ in range(n):
                rep.apply(refs[e], ("step",), [R8])
        if t in events:
            if mode != "run_kwin":
                assert eng.cell_layout() == (1 if resident else 0), (mode, t)      # straight after the launch: its plane is current
            for e in running_at[t]:
                assert refs[e].status()[0][0, 0] == 1, (t, e)
            for e in quit_at[t]:
                assert refs[e].status()[0][0, 0] == 0, (t, e)
            for envs, xy in events[t]:
                eng.reset_envs(envs, xy)
                for e, p in zip(envs, xy):                 # (in order: a later entry of the same environment replaces the earlier one)
                    logs[e] = [("table", 0), ("reset", p)]
                    refs[e] = rep.run(logs[e], [R8])
        for e in range(E):
            _check(eng, e, refs[e], (mode, t, e))


# ------------------------------------------------------------------ 2b. the full form (sf_reset) between episodes
FULL_CASES = {m: (m, None, False) for m in MODES}
FULL_CASES.update(fused0_then_run=("fused0", "run", False), run_then_fused0=("run", "fused0", False), run_arrival=("run", None, True))


@pytest.mark.parametrize("case", list(FULL_CASES))
def test_full_reset_between_episodes(case):
    """12 updates with control lines, a full ``reset`` with new ignitions, 12 more updates equal to the oracle after every call.
    Straight after the reset: the layout the full form chooses, ``run_cost`` zero, every result row that of update 0, the map
    delta exactly the ignition cell, arrival times 0 there and -1 elsewhere.  Two cases switch the launch structure in between:
    the layout choice is the branch only a full reset takes - the blocked plane iff the resident launch is what the handle will
    pick AND it stepped the handle last (or nothing has), so ``fused0 -> set_fused(2)`` starts the new episode on the row-major
    planes (the first resident launch converts them) and ``run -> set_fused(0)`` leaves the blocked plane."""
    mode, then, arrival = FULL_CASES[case]
    rng = np.random.default_rng(83500 + list(FULL_CASES).index(case))
    H, W = (150, 165) if mode in ("run_team", "run_win", "run_kwin") else (61, 83)
    E, md = 6, 4
    kw, R8 = _world(rng, H, W, md, True, diag=True)
    inits = [(int(rng.integers(W)), int(rng.integers(H))) for _ in range(E)]
    eng = _make(kw, E, mode, R8, inits)
    if mode != "run_kwin":
        assert eng.cell_layout() == (1 if mode in RESIDENT else 0)      # (a handle nothing has stepped yet: the automatic choice)
    if arrival:
        eng.enable_arrival(True)
    for e in range(E):
        eng.fire_map_delta(e)                               # (the first query sets the reference point up)
    rep = _Replay(kw, False, False)
    refs = {}

    def drive(n_updates, chunk, check):
        t = 0
        while t < n_updates:
            pts = _points(rng, E, H, W)
            if pts:
                eng.apply_mitigation(pts)
            n = min(chunk, n_updates - t)
            eng.step(n)
            t += n
            if check:
                for (e, x, y, ty) in pts:
                    rep.apply(refs[e], ("mit", [(x, y, ty)]), [R8])
                for e in range(E):
                    for _ in range(n):
                        rep.apply(refs[e], ("step",), [R8])
                    _check(eng, e, refs[e], (case, t, e))

    drive(12, 2 if mode in RESIDENT else 1, False)
    st = eng.status()[0]
    assert st[:, 1].max() > 0 and (st[:, 2] < H * W - 1).any()      # episodes under way: update() calls made, fires that spread
    if then:
        eng.set_fused(MODES[then]["fused"])
    inits = [(int(rng.integers(W)), int(rng.integers(H))) for _ in range(E)]
    eng.reset(inits)
    now = then or mode
    if now != "run_kwin":
        assert eng.cell_layout() == (1 if now in RESIDENT and mode in RESIDENT else 0), (case, eng.cell_layout())
    assert (eng.run_cost() == 0).all()
    st, el = eng.status()
    assert (st == np.array([1, 0, H * W - 1, 1, 0, 0, 0, 0])).all() and (el == 0).all(), (st, el)
    for e, (x, y) in enumerate(inits):
        idx, val = eng.fire_map_delta(e)
        assert idx.tolist() == [y * W + x] and val.tolist() == [1], (e, idx, val)      # exactly the ignition cell, BURNING
        if arrival:
            want = np.full((H, W), -1, dtype=np.int32)
            want[y, x] = 0
            assert (eng.arrival(e) == want).all(), e
    for e in range(E):
        refs[e] = rep.run([("table", 0), ("reset", inits[e])], [R8])
    drive(12, 2 if now in RESIDENT else 1, True)
    assert eng.status()[0][:, 1].max() > 0


def test_reset_refusals_change_nothing():
    """``reset_env`` before any ``reset`` is ``SF_ESTATE``; an ignition off the grid is ``SF_EINVAL`` from ``reset`` and ``reset_env``
    before anything is enqueued or switched: blobs, result block, ``run_cost`` and the layout - which the full reset would have
    changed here, the handle being told to step per update from now on - are what they were."""
    from simfire_amd._lib import SimfireHipError
    from simfire_amd.engine import FireEngine
    rng = np.random.default_rng(83900)
    H, W, E = 37, 101, 4
    kw, R8 = _world(rng, H, W, 4, True)
    inits = [(int(rng.integers(W)), int(rng.integers(H))) for _ in range(E)]
    fresh = FireEngine(n_envs=E, **kw)
    fresh.set_rtable(R8)
    with pytest.raises(SimfireHipError, match="sf_reset_env: call sf_reset once first"):
        fresh.reset_env(0, 1, 1)
    eng = _make(kw, E, "run", R8, inits)
    eng.step(6)
    eng.set_fused(0)
    assert eng.cell_layout() == 1
    was, st0, el0, cost0 = _blobs(eng), *eng.status(), eng.run_cost()
    for bad in ((W, 3), (5, -1)):
        xy = np.array(inits, dtype=np.int32)
        xy[2] = bad
        with pytest.raises(ValueError, match=r"reset: ignition \(%d, %d\) of environment 2 is outside the %dx%d grid" % (*bad, H, W)):
            eng.reset(xy)
        with pytest.raises(ValueError, match=r"reset: ignition \(%d, %d\) of environment 2 is outside" % bad):
            eng.reset_env(2, *bad)
        st, el = eng.status()
        assert _blobs(eng).tobytes() == was.tobytes() and (st == st0).all() and el.tobytes() == el0.tobytes(), bad
        assert eng.cell_layout() == 1 and (eng.run_cost() == cost0).all(), bad
    eng.reset(inits)                                         # (the same call with ignitions on the grid does switch)
    assert eng.cell_layout() == 0


# ------------------------------------------------------------------ 3. the mask form
def _mask_world(mode):
    """64 x 64, six environments with tables of their own: 0, 2 and 5 cannot spread (their fires are out after max_fire_duration
    updates), the others spread for ever.  Two handles alike, and the split checked with the oracle."""
    H = W = 64
    E, out = 6, [0, 2, 5]
    kw = dict(shape=(H, W), max_fire_duration=4, pixel_scale=50.0, update_rate=1.0, max_time=None, attenuate_line_ros=True,
              diagonal_spread=True)
    tabs = [np.full((8, H, W), 0.0 if e in out else 30.0) for e in range(E)]
    inits = [(20, 30)] * E
    for e in (0, 1):
        o = fire_dense.DenseOracle(**kw)
        o.set_rtable(tabs[e])
        o.reset([(20, 30)])
        o.step(6)
        assert o.status()[0][0, 0] == (0 if e == 0 else 1)
    a, b = (_make(kw, E, mode, tabs, inits, per_env=True) for _ in range(2))
    for x in (a, b):
        x.step(6)
    st = b.status()[0]
    assert sorted(np.flatnonzero(st[:, 0] == 0).tolist()) == out and (st[[1, 3, 4], 0] == 1).all()      # both kinds exist
    return a, b, kw, tabs, out


@pytest.mark.parametrize("mode", ["fused0", "run"])
def test_mask_form(mode):
    import torch
    a, b, kw, tabs, out = _mask_world(mode)
    E, W, H = 6, 64, 64
    rng = np.random.default_rng(84000)
    xy = np.stack([rng.integers(0, W, E), rng.integers(0, H, E)], axis=1).astype(np.int32)
    # not running, decided on the device
    done = np.flatnonzero(a.status()[0][:, 0] == 0)
    a.reset_envs(done, xy[done])
    b.reset_where(None, xy)
    _same(a, b, "reset_where(None)")
    assert (b.status()[0][:, 0] == 1).all()
    for x in (a, b):
        x.step(3)
    _same(a, b, "3 updates later")
    # an explicit mask that also selects running environments; bool and uint8; ignitions as a device tensor
    for dtype, sel in ((torch.uint8, [1, 2, 4]), (torch.bool, [0, 3])):
        mask = torch.zeros(E, dtype=dtype, device="cuda")
        mask[sel] = 1
        xy = np.stack([rng.integers(0, W, E), rng.integers(0, H, E)], axis=1).astype(np.int32)
        a.reset_envs(sel, xy[sel])
        b.reset_where(mask, torch.from_numpy(xy).cuda() if dtype is torch.bool else xy)
        _same(a, b, ("explicit mask", sel))
        for x in (a, b):
            x.step(2)
    # nothing selected: nothing changes
    was = _blobs(b)
    b.reset_where(torch.zeros(E, dtype=torch.uint8, device="cuda"), xy)
    now = _blobs(b)
    assert now.tobytes() == was.tobytes()
    # a device ignition off the grid: that environment is left as it is - not running -, the others are reset
    for x in (a, b):
        x.step(6)                                        # the fires of 0, 2, 5 are out again
    done = np.flatnonzero(a.status()[0][:, 0] == 0)
    assert len(done) >= 2
    bad = int(done[1])
    was = _blobs(b)
    dxy = torch.from_numpy(xy).cuda()
    dxy[bad, 0] = W
    others = [int(e) for e in done if e != bad]
    a.reset_envs(others, xy[others])
    b.reset_where(None, dxy)
    now = _same(a, b, "ignition off the grid")
    assert now[bad].tobytes() == was[bad].tobytes()
    st = b.status()[0]
    assert st[bad, 0] == 0 and (st[others, 0] == 1).all() and (st[others, 1] == 0).all()
    # ... and the episodes that follow are the oracle's
    for x in (a, b):
        x.step(4)
    for e in others:
        o = fire_dense.DenseOracle(**kw)
        o.set_rtable(tabs[e])
        o.reset([tuple(int(v) for v in xy[e])])
        o.step(4)
        _check(b, e, o, ("oracle", e))


def test_mask_form_takes_environments_that_quit_and_still_prune():
    """``prune_after_quit``: an environment that QUIT on the runtime check keeps pruning (its state word is 2) and its result row says
    not running - the maskless form takes it like the list built from the result block."""
    rng = np.random.default_rng(84500)
    H, W, E = 60, 70, 5
    kw, R8 = _world(rng, H, W, 4, True)
    kw.update(max_time=4.0, update_rate=1.0, pixel_scale=20.0)
    R8[:] = np.maximum(R8, 30.0)
    inits = [(int(rng.integers(W)), int(rng.integers(H))) for _ in range(E)]
    a, b = (_make(kw, E, "fused0", R8, inits, prune=True) for _ in range(2))
    for x in (a, b):
        x.step(4)
        x.reset_env(1, 9, 9)                                # (one environment younger than the others: still running below)
        x.step(3)
    st = a.status()[0]
    assert st[1, 0] == 1 and (st[[0, 2, 3, 4], 0] == 0).all() and (st[:, 3] > 0).all()      # QUIT with cells still burning: pruning goes on
    xy = np.stack([rng.integers(0, W, E), rng.integers(0, H, E)], axis=1).astype(np.int32)
    done = np.flatnonzero(st[:, 0] == 0)
    a.reset_envs(done, xy[done])
    b.reset_where(None, xy)
    _same(a, b, "prune_after_quit")
    for x in (a, b):
        x.step(5)
    _same(a, b, "prune_after_quit, 5 updates later")


# ------------------------------------------------------------------ 4. neighbours keep working
def test_fire_map_delta_after_a_batched_reset():
    rng = np.random.default_rng(85000)
    H, W, E = 70, 90, 4
    kw, R8 = _world(rng, H, W, 4, True)
    R8[:] = np.maximum(R8, 7.5)
    eng = _make(kw, E, "fused0", R8, [(10, 10), (20, 20), (30, 30), (40, 40)])
    for e in range(E):
        eng.fire_map_delta(e)                               # (the first query sets the reference point up)
    eng.step(5)
    for e in range(E):
        assert eng.fire_map_delta(e) is not None
    eng.step(2)
    eng.reset_envs([1, 3], [(17, 3), (0, 69)])
    for e, (x, y) in ((1, (17, 3)), (3, (0, 69))):
        idx, val = eng.fire_map_delta(e)
        assert idx.tolist() == [y * W + x] and val.tolist() == [1], (e, idx, val)      # exactly the ignition cell, BURNING
    assert eng.fire_map_delta(0) is not None                # an environment that was not reset keeps its reference point
    eng.step(3)
    eng.reset_where(None, np.array([(1, 1)] * E, dtype=np.int32))      # (whoever is selected, here nobody: the host cannot know)
    for e in range(E):
        assert eng.fire_map_delta(e) is None                # -1 once: fetch the whole map
    maps = eng.fire_maps().copy()
    eng.step(2)
    for e in range(E):
        idx, val = eng.fire_map_delta(e)                    # ... then deltas again
        m = maps[e].reshape(-1).copy()
        m[idx] = val
        assert (m.reshape(H, W) == eng.fire_map(e)).all(), e


@pytest.mark.parametrize("fused", [0, 2])
def test_observe_and_render_of_a_reset_environment(fused):
    import torch
    import test_observe_gpu as TO
    import test_render_gpu as TR
    eng, rng = TO._engine(90, 140, 4, 86000 + fused)
    eng.set_fused(fused)
    eng.step(7)
    assert eng.cell_layout() == (1 if fused == 2 else 0)
    eng.reset_envs([0, 2], [(139, 0), (64, 45)])
    TO._check(eng, agents=TO._agents(rng, 4, 90, 140))      # (observe first: it reads the plane the reset wrote)
    assert eng.fire_map(0)[0, 139] == 1 and (eng.fire_map(0) != 0).sum() == 1
    w = TR._World(90, 140, 4, 86100 + fused)
    w.eng.set_fused(fused)
    w.eng.step(7)
    mask = torch.tensor([0, 1, 0, 1], dtype=torch.uint8, device="cuda")
    w.eng.reset_where(mask, np.array([(0, 0), (3, 89), (5, 5), (128, 40)], dtype=np.int32))
    TR._check(w, agents=TR._agents(w.rng, 4, 90, 140))
    assert (w.eng.fire_map(3) != 0).sum() == 1 and w.eng.fire_map(3)[40, 128] == 1


@pytest.mark.parametrize("mode", ["fused1", "run"])
def test_clone_from_a_freshly_reset_environment(mode):
    rng = np.random.default_rng(87000)
    H, W, E = 80, 100, 4
    kw, R8 = _world(rng, H, W, 4, True)
    inits = [(int(rng.integers(W)), int(rng.integers(H))) for _ in range(E)]
    eng = _make(kw, E, mode, R8, inits)
    eng.step(6)
    eng.reset_envs([2], [(33, 44)])
    eng.copy_envs([2, 2], [0, 3])
    log = [("table", 0), ("reset", (33, 44))]
    rep = _Replay(kw, False, False)
    for t in range(8):
        eng.step(2)
        log += [("step",)] * 2
        ref = rep.run(log, [R8])
        for e in (0, 2, 3):
            _check(eng, e, ref, (mode, t, e))
    ref1 = rep.run([("table", 0), ("reset", inits[1])] + [("step",)] * 22, [R8])
    _check(eng, 1, ref1, "not reset")


def test_closed_loop_after_reset_done():
    """``reset_done`` with a mask, then a closed-loop episode against the oracle; ``reset_done`` while the loop runs ends it and
    still resets correctly."""
    import torch
    from test_env_state_gpu import _batched
    sim = _batched(4)
    eng = sim._engine
    H = W = 96
    kw = dict(shape=(H, W), max_fire_duration=int(eng.params.max_fire_duration), pixel_scale=float(eng.params.pixel_scale),
              update_rate=float(eng.params.update_rate), max_time=(float(eng.params.max_time) if eng.params.has_max_time else None),
              attenuate_line_ros=bool(eng.params.attenuate_line_ros), diagonal_spread=bool(eng.params.diagonal_spread))
    R8 = eng.get_rtable(0)
    orcs = []
    for e in range(4):
        o = fire_dense.DenseOracle(**kw)
        o.set_rtable(R8)
        o.reset([tuple(int(v) for v in sim.ignitions[e])])
        orcs.append(o)
    sim.run(9, return_maps=False)
    for o in orcs:
        o.step(9)
    sim.ignitions[1] = (80, 15)
    sim.ignitions[3] = (0, 95)
    sim.reset_done(torch.tensor([0, 1, 0, 1], dtype=torch.bool, device="cuda"))
    for e in (1, 3):
        orcs[e].reset([tuple(int(v) for v in sim.ignitions[e])])
    rng = np.random.default_rng(88000)

    def episode(n):
        for _ in range(n):
            pts = np.stack([rng.integers(0, W, (4, 2)), rng.integers(0, H, (4, 2)), rng.integers(3, 6, (4, 2))], axis=2).astype(np.int32)
            rows, el = sim.loop_step(pts)
            for e in range(4):
                orcs[e].apply_mitigation([(0, int(x), int(y), int(ty)) for (x, y, ty) in pts[e]])
                orcs[e].step(1)
                so, eo = orcs[e].status()
                assert (rows[e] == so[0]).all() and el[e] == eo[0], (e, rows[e], so[0])

    sim.loop_start(2)
    episode(7)
    sim.ignitions[0] = (50, 50)
    sim.reset_done(torch.tensor([1, 0, 0, 0], dtype=torch.uint8, device="cuda"))      # the loop is running: it is ended first
    orcs[0].reset([(50, 50)])
    with pytest.raises(Exception, match="loop_start"):
        eng.loop_step(None)
    for e in range(4):
        _check(eng, e, orcs[e], ("after reset_done in the loop", e))
    sim.loop_start(2)
    episode(5)
    sim.loop_stop()
    for e in range(4):
        _check(eng, e, orcs[e], ("at the end", e))


# ------------------------------------------------------------------ 5. seeds through the one batched call
@pytest.mark.parametrize("kind", [0, 2])
def test_layer_seeds_and_reset_of_a_list(kind):
    import test_layer_gen_gpu as TL
    from simfire_amd.config import Config
    from simfire_amd.simulation import BatchedFireSimulation
    H, W, E = 128, 144, 6
    listed = [1, 3, 4]
    default = (827, 1113, 2345, 650)
    seeds = [((11 * e - 20, 1113 + e, 300 + 7 * e, 650 - 3 * e) if e in listed else default) for e in range(E)]
    sim = BatchedFireSimulation(Config(config_dict=TL._dict(H, W), simplex_topography=True), E, per_env_terrain=True)
    sim._engine.set_fused(kind)
    sim.run(10, return_maps=False)
    assert sim.set_seeds({"elevation": [seeds[e][0] for e in listed], "fuel": [seeds[e][1] for e in listed],
                          "wind_speed": [seeds[e][2] for e in listed], "wind_direction": [seeds[e][3] for e in listed]}, envs=listed) is True
    calls = {"reset_envs": 0, "reset_env": 0}
    for name in calls:
        def counted(*a, _f=getattr(sim._engine, name), _n=name, **k):
            calls[_n] += 1
            return _f(*a, **k)
        setattr(sim._engine, name, counted)
    sim.reset(listed)
    assert calls == {"reset_envs": 1, "reset_env": 0}
    host = TL._host_batch(H, W, seeds, None, ignitions=sim.ignitions.copy())
    host._engine.set_fused(kind)
    for e in listed:
        assert sim._engine.get_rtable(e).tobytes() == host._engine.get_rtable(e).tobytes()
    for it in range(3):
        sim.run(12, return_maps=False)
        host.run(12, return_maps=False)
        sa, ea = sim.results()
        sb, eb = host.results()
        np.testing.assert_array_equal(sa[listed], sb[listed])
        assert ea[listed].tobytes() == eb[listed].tobytes()
        for e in listed:
            assert sim._engine.fire_map(e).tobytes() == host._engine.fire_map(e).tobytes(), (it, e)
            assert sim._engine.burn(e).tobytes() == host._engine.burn(e).tobytes(), (it, e)
    assert sim.results()[0][listed, 1].min() > 0


# ------------------------------------------------------------------ 6. async mode
@pytest.mark.parametrize("mode", ["fused0", "run"])
def test_async_mode(mode):
    rng = np.random.default_rng(89000)
    H, W, E = 120, 130, 5
    kw, R8 = _world(rng, H, W, 4, True)
    inits = [(int(rng.integers(W)), int(rng.integers(H))) for _ in range(E)]
    a, b = (_make(kw, E, mode, R8, inits) for _ in range(2))
    b.set_async(True)
    for x in (a, b):
        x.step(8)
        x.reset_envs([4, 0], [(129, 119), (16, 7)])
        x.step(5)
        x.reset_envs([1], [(3, 3)])
        x.reset_envs([2, 1], [(64, 64), (15, 100)])      # back to back: the second call's list follows the first through the pinned buffer
        x.step(3)
    b.sync()
    _same(a, b, "async")


if __name__ == "__main__":
    print("PARENT = {")
    for ci, case in enumerate(CASES):
        for mi, mode in enumerate(MODES):
            print(f"    ({case!r}, {mode!r}): {_twin_world(81000 + 17 * ci + mi, mode, **CASES[case])[0]!r},", flush=True)
    for mode in MODES_1024:
        print(f"    ('1024', {mode!r}): {_twin_world(82000 + len(mode), mode, **CASE_1024)[0]!r},", flush=True)
    print("}")
