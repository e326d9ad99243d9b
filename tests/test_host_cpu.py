"""CPU tests of the host side: config / units / sharding logic, the C-ABI surface, and the
world_size-2 path over gloo (with the C oracle standing in for the GPU engine)."""
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tests", "golden", "configs")


def test_units():
    from simfire_amd.units import meters_to_feet, mph_to_ftpm, str_to_minutes
    assert mph_to_ftpm(7) == 616 and meters_to_feet(100) == 328.084
    assert [str_to_minutes(s) for s in ["24h", "1h", "2d 3h", "90", "1h 60m", "1.5h", "120m", "45s"]] == \
        [1440, 60, 3060, 90, 120, 90, 120, 1]


def test_config_flat_simple():
    """simfire/utils/_tests/test_configs/test_config_flat_simple.yml as the reference loads it."""
    from simfire_amd.config import Config
    c = Config(os.path.join(CFG, "test_config_flat_simple.yml"))
    assert c.area.screen_size == (9, 9) and c.area.pixel_scale == 50.0
    assert c.simulation.update_rate == 1.0 and c.simulation.runtime == 1440
    assert c.mitigation.ros_attenuation is True
    assert c.fire.fire_initial_position == (5, 3) and c.fire.max_fire_duration == 4 and c.fire.diagonal_spread
    assert c.environment.moisture == 0.03
    assert c.wind.speed.shape == (9, 9) and c.wind.speed.dtype == np.float64 and (c.wind.speed == 616.0).all()
    assert (c.wind.direction == 90.0).all()
    assert c.terrain.topography_layer.data.shape == (9, 9, 1) and not c.terrain.topography_layer.data.any()
    f = c.terrain.fuel_layer.data[0, 0, 0]
    # chaparral(seed=1113): legacy np.random.seed + uniform per field (utils/terrain.py:29-114)
    assert (f.w_0, f.delta, f.M_x, f.sigma) == (0.9810356625846572, 5.890006842991012, 0.9833113830744984,
                                                3433.643783383716)


def test_config_gaussian_and_errors():
    from simfire_amd.config import Config, ConfigError
    import yaml
    # this fixture asks for perlin wind: the fields come from the build's own simplex generator with the fixture's parameters
    # (config.py:892-929; generator parity unpinned - the `noise` wheel is absent and the reference pins no wind value)
    cp = Config(os.path.join(CFG, "test_config_gaussian.yml"))
    g = yaml.safe_load(open(os.path.join(CFG, "test_config_gaussian.yml")))
    ps, pd = g["wind"]["perlin"]["speed"], g["wind"]["perlin"]["direction"]
    assert cp.wind.speed.dtype == np.float64 and cp.wind.speed.shape == cp.area.screen_size == cp.wind.direction.shape
    assert cp.wind.speed.min() >= ps["range_min"] * 88.0 - 1e-3 and cp.wind.speed.max() <= ps["range_max"] * 88.0 + 1e-3 and cp.wind.speed.std() > 0
    assert cp.wind.direction.min() >= pd["range_min"] and cp.wind.direction.max() <= pd["range_max"]      # the reference's own test is this range check (test_wind.py:27-37)
    assert cp.wind.speed_function.name == "perlin" and cp.wind.speed_function.kwargs["seed"] == ps["seed"]
    before = cp.wind.speed.copy()
    cp.reset_wind(speed_seed=ps["seed"] + 1)                   # config.py:1048-1086
    assert cp.yaml_data["wind"]["perlin"]["speed"]["seed"] == ps["seed"] + 1 and not (cp.wind.speed == before).all()
    cp.reset_wind(speed_seed=ps["seed"])
    assert (cp.wind.speed == before).all()                     # deterministic in the seed
    g["wind"]["function"] = "cfd"
    with pytest.raises(ConfigError):
        Config(config_dict=g)
    g["wind"]["function"] = "simple"
    c = Config(config_dict=g)
    H, W = c.area.screen_size
    el = c.terrain.topography_layer.data.squeeze()
    assert el.shape == (H, W) and el.max() <= 500 and el.min() >= 0 and el.std() > 0
    with pytest.raises(ValueError):
        Config()
    with pytest.raises(ConfigError):
        Config(os.path.join(CFG, "does_not_exist.yml"))
    d = yaml.safe_load(open(os.path.join(CFG, "functional_config.yml")))
    with pytest.raises(ConfigError):           # perlin topography needs the `noise` wheel
        Config(config_dict=d)
    d["terrain"]["topography"]["functional"]["function"] = "flat"
    d["fire"]["fire_initial_position"]["type"] = "random"
    c = Config(config_dict=d)
    rng = np.random.default_rng(1234)
    assert c.fire.fire_initial_position == (int(rng.integers(225, dtype=int)), int(rng.integers(225, dtype=int)))
    assert c.fire.seed == 1234


def test_config_from_arrays():
    import yaml
    from simfire_amd.config import Config
    from simfire_amd.parameters import FuelModelToFuel
    d = yaml.safe_load(open(os.path.join(CFG, "test_config_flat_simple.yml")))
    codes = np.array([[1, 4, 98], [10, 13, 2]])
    c = Config.from_arrays(d, codes, np.zeros((2, 3)), np.full((2, 3), 100.0), np.full((2, 3), 45.0))
    assert c.area.screen_size == (2, 3)
    assert c.terrain.fuel_layer.data[0, 2, 0] is FuelModelToFuel[98]
    assert c.wind.speed[1, 1] == 100.0


def test_shard_envs():
    from simfire_amd.parallel import shard_envs
    for n, w in [(1024, 8), (10, 3), (5, 8), (256, 1)]:
        spans = [shard_envs(n, r, w) for r in range(w)]
        assert spans[0][0] == 0 and spans[-1][1] == n
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
        sizes = [b - a for a, b in spans]
        assert max(sizes) - min(sizes) <= 1


def test_c_abi_exports_every_declared_symbol():
    """The shared library loads (no GPU needed for that) and exports every function that include/simfire_hip.h (the boundary a
    SimFire maintainer binds) and include/simfire_hip_lab.h (knobs, counters, introspection: bench / tests / profiles) declare;
    the ctypes table binds exactly that set; the boundary header holds no laboratory entry."""
    from simfire_amd import _lib
    header = open(os.path.join(ROOT, "include", "simfire_hip.h")).read()
    lab = open(os.path.join(ROOT, "include", "simfire_hip_lab.h")).read()
    strip = lambda h: re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    boundary = set(re.findall(r"\b(sf_[a-z_0-9]+)\s*\(", strip(header)))
    laboratory = set(re.findall(r"\b(sf_[a-z_0-9]+)\s*\(", strip(lab)))
    assert not (boundary & laboratory)
    assert "No reference counterpart" not in header and "sf_set_tuning" not in boundary and "sf_get_run_cost" not in boundary
    declared = boundary | laboratory
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name), name
    assert declared == set(_lib.SIGNATURES) | set(_lib.STRING_GETTERS)
    assert lib.sf_version().decode().startswith("simfire_hip")


def test_product_has_no_oracle_or_cpu_fallback():
    """The product package must not import the oracle (test infrastructure)."""
    pkg = os.path.join(ROOT, "simfire_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            src = open(os.path.join(pkg, fn)).read()
            assert "oracle" not in src.replace("the oracle", "").replace("C oracle", ""), fn


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


WORKER = r'''
import os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch, torch.distributed as dist
from oracle import fire_dense
from simfire_amd import workloads
from simfire_amd.parallel import shard_envs, gather_results
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
n_total = 5                                   # ragged: 3 + 2
lo, hi = shard_envs(n_total, rank, world)
w = workloads.c3(64, n_total)                 # every rank sees the same global ignition list
kw = w.engine_kwargs(); kw["n_envs"] = hi - lo
o = fire_dense.DenseOracle(**kw)
o.build_rtable(w.w_0, w.delta, w.M_x, w.sigma, w.elevation, w.U, w.U_dir, w.M_f)
o.reset(w.init_xy[lo:hi])
o.step(40)
block = torch.from_numpy(o.status()[0].copy())
allb = gather_results(block)
if rank == 0:
    kw["n_envs"] = n_total
    ref = fire_dense.DenseOracle(**kw)
    ref.build_rtable(w.w_0, w.delta, w.M_x, w.sigma, w.elevation, w.U, w.U_dir, w.M_f)
    ref.reset(w.init_xy)
    ref.step(40)
    assert allb.shape == (n_total, 8), allb.shape
    assert (allb.numpy() == ref.status()[0]).all()
    print("GATHER_OK")
dist.barrier()
dist.destroy_process_group()
'''


def test_two_rank_gloo_shard_and_gather(tmp_path):
    """N > 1 path on CPU: env axis sharded over 2 ranks (ragged 3 + 2), no data-path collective,
    one all-gather of the result blocks - equals the single-process run."""
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, str(script), ROOT], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=240)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert "GATHER_OK" in outs[0]


def test_missing_extension_fails_loudly(monkeypatch):
    """No CPU fallback: without the HIP library the product path raises, it does not degrade."""
    from simfire_amd import _lib
    monkeypatch.setattr(_lib, "_libs", {})
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libsimfire_hip.so")
    with pytest.raises(_lib.SimfireHipError):
        _lib.load()
    from simfire_amd.engine import FireEngine
    with pytest.raises(_lib.SimfireHipError):
        FireEngine((8, 8))


def test_error_code_mapping():
    from simfire_amd import _lib
    lib = _lib.load()
    # argument validation happens before any HIP call, so these work without a GPU
    import ctypes as C
    p = _lib.SfParams(n_envs=0, height=4, width=4, max_fire_duration=4, diagonal_spread=1, attenuate_line_ros=1,
                      has_max_time=0, device=0, pixel_scale=1.0, update_rate=1.0, max_time=0.0, h=8000, S_T=0.0555,
                      S_e=0.01, p_p=32, M_f=0.03)
    h = C.c_void_p()
    rc = lib.sf_create(C.byref(p), C.byref(h))
    assert rc == _lib.SF_EINVAL
    with pytest.raises(ValueError):
        _lib.check(rc)
    p.n_envs, p.max_fire_duration = 1, 29
    rc = lib.sf_create(C.byref(p), C.byref(h))
    assert rc == _lib.SF_ENOTSUP
    with pytest.raises(NotImplementedError):
        _lib.check(rc)
    assert b"max_fire_duration" in lib.sf_last_error()


def test_bench_self_launch_plumbing():
    """`python bench.py --gpus 2` outside a launcher starts its two ranks itself (RANK / WORLD_SIZE / MASTER_*), they
    rendezvous (gloo here: no GPU in this container), all-gather a result block and rank 0 prints ONE JSON line
    with n_gpus = 2; under an existing launcher environment it uses the ranks it is given."""
    import json
    bench = os.path.join(ROOT, "bench.py")
    out = subprocess.run([sys.executable, bench, "--gpus", "2", "--plumbing-only", "--envs", "3"], capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["gathered_rows"] == 6 and j["ok"] is True
    one = subprocess.run([sys.executable, bench, "--plumbing-only", "--envs", "3"], capture_output=True, text=True, timeout=300)
    assert json.loads([l for l in one.stdout.splitlines() if l.startswith("{")][0])["n_gpus"] == 1
    # --scaling strong: --envs is the TOTAL, split over the ranks in contiguous blocks of the env axis
    strong = subprocess.run([sys.executable, bench, "--gpus", "2", "--plumbing-only", "--scaling", "strong", "--envs", "6"], capture_output=True,
                            text=True, timeout=300)
    assert strong.returncode == 0, strong.stdout + strong.stderr
    j = json.loads([l for l in strong.stdout.splitlines() if l.startswith("{")][0])
    assert j["n_gpus"] == 2 and j["gathered_rows"] == 6 and j["ok"] is True
    odd = subprocess.run([sys.executable, bench, "--gpus", "2", "--plumbing-only", "--scaling", "strong", "--envs", "5"], capture_output=True,
                         text=True, timeout=300)
    assert odd.returncode != 0 and "do not split evenly" in odd.stderr


def test_bench_dump_outputs_are_float_seeded_and_within_64_mb(tmp_path):
    """bench.py --dump-outputs on a stand-in engine (the GPU test checks the values): float32 / float64 files, at most 64 MB for C3's
    and C4's grids and for a grid of which not even one environment fits (then a seeded sample of cells), the same sample every run."""
    import bench

    class Stub:
        def __init__(self, H, W, E):
            self.H, self.W, self.n_envs = H, W, E

        def fire_map(self, e):
            return (np.arange(self.H * self.W).reshape(self.H, self.W) * (e + 1) % 6).astype(np.uint8)

        def burn(self, e):
            return np.full((self.H, self.W), float(e))

        def status(self):
            return np.zeros((self.n_envs, 8), np.int32), np.arange(self.n_envs, dtype=np.float64)

    for H, W, E in ((1024, 1024, 256), (2048, 2048, 128), (4096, 4096, 2)):
        runs = []
        for k in range(2):
            d = tmp_path / f"{H}_{k}"
            names = bench.dump_outputs(Stub(H, W, E), np.ones((E, 8), np.int32), str(d))
            arrs = {n: np.load(d / f"{n}.npy") for n in names}
            assert sum(os.path.getsize(d / f"{n}.npy") for n in names) <= 64 << 20
            assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
            runs.append(arrs)
        assert all((runs[0][n] == runs[1][n]).all() for n in runs[0])
        envs = runs[0]["sample_envs"].astype(int)
        fm = runs[0]["fire_map"].reshape(len(envs), -1)
        cells = runs[0]["sample_cells"].astype(np.int64) if "sample_cells" in runs[0] else np.arange(H * W)
        assert (H * W > 4 << 20) == ("sample_cells" in runs[0])
        for i, e in enumerate(envs):
            assert (fm[i] == Stub(H, W, E).fire_map(e).ravel()[cells]).all()


@pytest.mark.parametrize("data_type", ["npy", "jsonl", "json", "h5"])
def test_savedata_writer_against_the_reference_run(tmp_path, data_type, monkeypatch):
    """simfire_amd/savedata.py (host code) fed the per-update maps and observation planes the REFERENCE produced
    (tests/golden/save_data_c1_32.npz, recorded by make_golden_savedata.py) in two run() calls of 7 and 5 updates:
    file list, metadata and history of simulation.py:887-959, 1059-1104 for every data_type."""
    import json
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _golden
    import _h5
    from simfire_amd.savedata import write_history
    if data_type == "h5":
        h5py = _h5.h5py_module(monkeypatch)            # (the real h5py, or tests/_h5.py's stand-in where it is not installed)
    d = _golden.load("save_data_c1_32.npz")
    names = [str(n) for n in d["static_names"]]
    static = {n: d[f"attr_{n}"] for n in names}
    meta = {"config": {"area": {"screen_size": [32, 32]}}, "seeds": {"elevation": None}, "layer_types": {"fuel": "functional"}}
    hist = d["history"].astype(np.int64)
    write_history(tmp_path, data_type, hist[:7], 0, static, meta)
    write_history(tmp_path, data_type, hist[7:], 7, static, meta)
    ext = {"npy": "npy", "h5": "h5"}.get(data_type, "jsonl")
    sext = {"npy": "npy", "h5": "h5"}.get(data_type, "json")
    assert sorted(os.listdir(tmp_path)) == sorted([f"fire_map.{ext}", "metadata.json"] + [f"{n}.{sext}" for n in names])
    m = json.load(open(tmp_path / "metadata.json"))
    assert list(m) == ["config", "seeds", "layer_types", "shape", "static_data", "fire_map"]      # the reference's key order
    assert sorted(m) == [str(k) for k in d["metadata_keys"]]
    assert m["shape"] == [int(v) for v in d["metadata_shape"]] and m["fire_map"] == f"fire_map.{ext}"
    if data_type == "npy":
        assert sorted(os.listdir(tmp_path)) == [str(f) for f in d["files"]]
        assert m["static_data"] == json.loads(str(d["metadata_static"])) and m["fire_map"] == str(d["metadata_fire_map"])
        got = np.load(tmp_path / "fire_map.npy")
        assert got.dtype == np.int8 and (got == d["history"]).all()
        for n, dt in zip(names, d["static_dtypes"]):
            a = np.load(tmp_path / f"{n}.npy")
            assert (a == static[n]).all() and str(a.dtype) == str(static[n].dtype)
    elif data_type == "h5":
        with h5py.File(tmp_path / "fire_map.h5", "r") as f:
            assert (np.asarray(f["data"]) == d["history"]).all()
    else:
        lines = open(tmp_path / "fire_map.jsonl").read().splitlines()
        assert [list(json.loads(ln)) for ln in lines] == [[str(i + 1)] for i in range(12)]
        assert all((np.array(json.loads(ln)[str(i + 1)]) == d["history"][i]).all() for i, ln in enumerate(lines))
        for n in names:
            assert (np.array(json.load(open(tmp_path / f"{n}.json"))["data"]) == static[n]).all()
    with pytest.raises(ValueError):
        write_history(tmp_path, "csv", hist[:1], 12, static, meta)


def test_layer_fingerprint_sees_every_element():
    """the change test of FireSimulation.reset must see an edit of ANY element - the reference's reset() rebuilds terrain
    and fire manager every time (simulation.py:202-214).  A strided sample (stride 16 at 1024^2) missed columns 1..15."""
    from simfire_amd.simulation import _fingerprint
    a = np.zeros((1024, 1024))
    f0 = _fingerprint(a)
    a[:, 1:15] = 3.0
    f1 = _fingerprint(a)
    a[777, 9] = 4.0
    f2 = _fingerprint(a)
    assert len({f0, f1, f2}) == 3
    b = np.zeros((1024, 1024), dtype=np.float32)
    assert _fingerprint(b) != f0                               # dtype takes part
    assert _fingerprint(a.copy()) == f2                        # contents, not identity
