"""Probe: environment state (sf_copy_envs / sf_save_state / sf_load_state, simfire_amd/csrc/sf_state_kernels.h).
Writes profiles/state_fork_timing.txt in two steps:

  python profiles/state_probe.py OUT.txt                       # items 1-4 below (wall clock, HIP events), OUT.txt rewritten
  rocprofv3 --kernel-trace --stats -d DIR -o run -- python profiles/state_probe.py --fork-only
  python profiles/state_probe.py --rocprof DIR/run_results.db OUT.txt      # appends item 5: the same fork as the profiler saw it

1. Fork 1 -> 63 on C3's 64 x 1024^2 mid-episode (after 30 updates of the resident launch: the blocked plane is current): bytes
   each destination receives (from the handle's shapes), wall time of sf_copy_envs; then the same bytes as 63 hipMemcpyAsync
   device-to-device copies from one source buffer (the same one-to-many pattern), on one stream, in the same run (HIP events).
2. The step launch right after a fork against one without, C3 256 x 1024^2 stepping 20 updates per call (k_run, after the fires
   have outgrown the window phase): 7 alternating trials each, kernel milliseconds from sf_step_timed.
3. save_state / load_state of one 1024^2 environment, to a device buffer and to the host (median of 7).
4. copy.deepcopy(FireSimulation) at 1024^2 (median of 3).
5. (--rocprof) k_env_copy per dispatch and the runtime's copy kernel (__amd_rocclr_copyBuffer) per hipMemcpyAsync, from the
   profiler's database of the --fork-only run (5 forks, 5 x 63 copies).
"""
import copy
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from simfire_amd import workloads  # noqa: E402
from simfire_amd.engine import FireEngine  # noqa: E402


def engine(E, size=1024):
    w = workloads.c3(size, E)
    eng = FireEngine(**w.engine_kwargs())
    eng.set_layers(*w.layers())
    eng.reset(w.init_xy)
    return w, eng


def copied_bytes(eng, w):
    """Bytes sf_copy_envs writes per destination on a handle whose blocked plane is current."""
    H, W = w.shape
    g = eng.geometry()
    P = g["pitch"]
    PV = P // 16
    cells = ((H + 3) // 4 + 2) * PV * 128
    plane = H * P
    VW = (PV + 63) // 64
    tiles = g["tiles_x"] * g["tiles_y"]
    chunks = -(-PV // (g["tile_w"] // 16))
    Hs = (H + 512 + 16 + 7) // 8 * 8
    seam = (chunks + 1) * 2 * Hs
    tf = 2 * (g["tiles_y"] + 2) * (g["tiles_x"] + 2)
    parts = dict(cells=cells, burn=8 * plane, settled=4 * plane if w.attenuate_line_ros else 0, vbits=3 * H * VW * 8, seam=seam,
                 tiles=tiles * 17 + tf, scalars=24 + 32 + 8 + 8 + 4)
    return sum(parts.values()), parts


def hip_memcpy_ms(dst_ptrs, src_ptr, nbytes, reps=5):
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    stream = torch.cuda.current_stream().cuda_stream
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for d in dst_ptrs:
            assert hip.hipMemcpyAsync(C.c_void_p(d), C.c_void_p(src_ptr), nbytes, 3, C.c_void_p(stream)) == 0
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def fork(out):
    w, eng = engine(64)
    eng.step(30)
    nb, parts = copied_bytes(eng, w)
    rest = list(range(1, 64))
    ts = []
    for _ in range(5):
        eng.sync()
        t0 = time.perf_counter()
        eng.copy_envs([0] * 63, rest)          # (synchronous: returns when the launch has finished)
        ts.append((time.perf_counter() - t0) * 1e3)
    wall = statistics.median(ts)
    src = torch.empty(nb, dtype=torch.uint8, device="cuda")
    dst = torch.empty((63, nb), dtype=torch.uint8, device="cuda")
    mc = hip_memcpy_ms([dst[i].data_ptr() for i in range(63)], src.data_ptr(), nb)
    out.append("1. fork 1 -> 63, C3 64 x 1024^2 after 30 updates (blocked plane current)")
    out.append(f"  bytes per destination {nb} ({', '.join(f'{k} {v}' for k, v in parts.items())})")
    out.append(f"  bytes written in all  {63 * nb} ({63 * nb / 1e9:.3f} GB; the source is read 63 times)")
    out.append(f"  sf_copy_envs wall     {wall:.3f} ms (median of 5, host validation + launch + wait)")
    out.append(f"  63 x hipMemcpyAsync   {mc:.3f} ms (HIP events, median of 5) = {63 * nb / mc / 1e6:.0f} GB/s written")
    return eng


def step_after_fork(out):
    w, eng = engine(256)
    eng.step(100)                              # fires past the window phase
    ts = {"fork": [], "none": []}
    for trial in range(14):
        kind = "fork" if trial % 2 == 0 else "none"
        if kind == "fork":
            eng.copy_envs([0], [1])
        eng.sync()
        ts[kind].append(eng.step_timed(20))
    out.append("2. step launch after a fork, C3 256 x 1024^2, step(20) after 100 updates (k_run), kernel ms, 7 alternating trials each")
    for k in ("fork", "none"):
        v = ts[k]
        out.append(f"  {k:5s} median {statistics.median(v):.3f}  range {min(v):.3f} - {max(v):.3f}   {' '.join(f'{x:.3f}' for x in v)}")


def save_load(out):
    w, eng = engine(1)
    eng.step(40)
    nb = eng.state_bytes()
    dev = torch.empty(nb, dtype=torch.uint8, device="cuda")
    res = {}
    for name, fn in (("save device", lambda: eng.save_state([0], out=dev)), ("load device", lambda: eng.load_state([0], dev)),
                     ("save host", lambda: eng.save_state([0])), ("load host", lambda: eng.load_state([0], host))):
        if name == "load host":
            host = eng.save_state([0])
        ts = []
        for _ in range(8):
            eng.sync()
            t0 = time.perf_counter()
            fn()
            eng.sync()
            ts.append((time.perf_counter() - t0) * 1e3)
        res[name] = statistics.median(ts[1:])
    out.append(f"3. save_state / load_state, one 1024^2 environment, blob {nb} bytes, wall ms (median of 7 after one warm-up)")
    for k, v in res.items():
        out.append(f"  {k:12s} {v:.3f} ms")


def deepcopy_sim(out):
    import yaml
    from simfire_amd.config import Config
    from simfire_amd.simulation import FireSimulation
    y = yaml.safe_load(open(os.path.join(ROOT, "tests", "golden", "configs", "functional_config.yml")))
    y["area"]["screen_size"] = [1024, 1024]
    y["terrain"]["topography"]["functional"]["function"] = "flat"
    y["simulation"]["headless"] = True
    sim = FireSimulation(Config(config_dict=y))
    sim.run(20)
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        twin = copy.deepcopy(sim)
        ts.append((time.perf_counter() - t0) * 1e3)
        twin._engine.close()
    out.append(f"4. copy.deepcopy(FireSimulation) at 1024^2 after 20 updates: {statistics.median(ts):.1f} ms wall (median of 3: "
               f"{' '.join(f'{t:.1f}' for t in ts)})")


def rocprof(db, path):
    """Item 5 from a rocprofv3 database (rocpd SQLite) of the --fork-only run, appended to the file item 1 wrote."""
    import re
    import sqlite3
    text = open(path).read()
    total = int(re.search(r"bytes written in all\s+(\d+)", text).group(1))
    c = sqlite3.connect(db)
    rows = c.execute("select duration, grid_x, grid_y, workgroup_x, vgpr_count, scratch_size from kernels where name like '%k_env_copy%'").fetchall()
    dur = [r[0] / 1e3 for r in rows]
    cp = [r[0] / 1e3 for r in c.execute("select duration from kernels where name like '%rocclr_copyBuffer%'").fetchall()]
    med = statistics.median(dur)
    per63 = 63 * statistics.median(cp)
    g = rows[0]
    out = [f"5. rocprofv3 --kernel-trace (the --fork-only run: {len(dur)} forks, {len(cp)} runtime copy dispatches)",
           f"  k_env_copy            {med:.2f} us median of {len(dur)} ({min(dur):.2f} - {max(dur):.2f}), grid {g[1] // g[3]} x {g[2]} workgroups "
           f"of {g[3]} lanes, {g[4]} VGPRs, scratch {g[5]} = {total / med / 1e6:.2f} TB/s written",
           f"  __amd_rocclr_copyBuffer {statistics.median(cp):.2f} us median per hipMemcpyAsync, {per63:.1f} us per 63",
           f"  ratio k_env_copy / the 63 copies = {med / per63:.2f}  (target: within 1.25x)"]
    with open(path, "a") as f:
        f.write("\n".join(out) + "\n")
    print("\n".join(out))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--rocprof" in sys.argv:
        rocprof(args[0], args[1])
        return
    out = []
    fork(out)
    if "--fork-only" in sys.argv:
        print("\n".join(out))
        return
    step_after_fork(out)
    save_load(out)
    deepcopy_sim(out)
    path = args[0] if args else os.path.join(ROOT, "profiles", "state_fork_timing.txt")
    head = ["Environment state on one MI355X: written by profiles/state_probe.py (items 1-4; item 5 appended by its --rocprof step)."]
    with open(path, "w") as f:
        f.write("\n".join(head + out) + "\n")
    print("\n".join(out))


if __name__ == "__main__":
    main()
