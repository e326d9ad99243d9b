"""Probe: what a wind change during an episode costs (sf_set_wind / sf_set_wind_schedule, simfire_amd/csrc/sf_wind_kernels.h;
DESIGN.md section 18).  Per-environment terrain, C3's layers in every table; 7 runs after one warm-up run, median [min, max].

  (a) the only route before this feature: generate_layers with constant wind and every other plane left alone - a synchronous call,
      timed by the host clock around it - plus the k_rt_cellmajor pass the next resident launch pays: the host time of step(2)
      behind it minus the host time of the same step(2) with the cell-major copy current,
  (b) sf_set_wind, uniform wind, cache warm                      - GPU time by HIP events around its launches (sf_set_wind_lab),
  (c) sf_set_wind with a device field [n][H][W]                  - the same,
  (d) the same kernel computing its terms from the layers (cache switched off: the cache-fill path) - the same,
  (e) the schedule pass with nothing due (memset + k_wind_due + an empty k_wind_rtable) - the same,
  (f) a synchronous 1-update sf_step with a schedule set but nothing due and without one, over the same tables and the same fires (the
      pass stands in front of where a timed call's events begin, so: host clock around 20 calls, per call); with SIMFIRE_HIP_PARENT
      (default profiles/_variants/libsimfire_hip_parent.so) the same on the parent commit's library.

  python profiles/wind_probe.py            # 1024^2 x 256 and 225^2 x 4 -> profiles/wind_change_timing.txt
  python profiles/wind_probe.py --quick    # 225^2 x 4 only, nothing written"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "profiles", "wind_change_timing.txt")
PARENT = os.environ.get("SIMFIRE_HIP_PARENT") or os.path.join(ROOT, "profiles", "_variants", "libsimfire_hip_parent.so")
REPS = 7
NEW = ("sf_set_wind", "sf_set_wind_schedule", "sf_set_wind_lab", "sf_get_wind_ms")


def _engine(size, E):
    from simfire_amd import workloads
    from simfire_amd.engine import FireEngine
    w = workloads.c3(size, E)
    eng = FireEngine(per_env_terrain=True, **w.engine_kwargs())
    eng.set_layers(*w.layers())
    return eng, w.init_xy


def child_parent(size, E):
    from simfire_amd import _lib
    for name in NEW:
        _lib.SIGNATURES.pop(name, None)
    eng, xy = _engine(size, E)
    eng.generate_layers(list(range(E)), wind_speed=1760.0, wind_direction=90.0)      # (the tables of the schedule's first row)
    ms = [step1_us(eng, xy) for rep in range(REPS + 1)]
    print("RESULT " + json.dumps(dict(f_parent=ms[1:])))


def step1_us(eng, xy):
    """Host microseconds per synchronous step(1), 20 in a row, after 20 + 1 updates from a reset (no buffer is left to rebuild)."""
    eng.reset(xy)
    eng.step(20)
    eng.step(1)
    eng.sync()
    t0 = time.perf_counter()
    for _ in range(20):
        eng.step(1)
    eng.sync()
    return (time.perf_counter() - t0) / 20 * 1e6


def child(size, E):
    import numpy as np
    import torch
    eng, xy = _engine(size, E)
    envs = list(range(E))
    res = {k: [] for k in ("a_gen", "a_rtc", "b", "c", "d", "e", "f_off", "f_on")}
    dev = f"cuda:{eng.params.device}"
    U = np.linspace(900.0, 2600.0, E)
    D = np.linspace(0.0, 350.0, E)
    fu = torch.rand((E, size, size), dtype=torch.float64, device=dev) * 2000.0 + 300.0
    fd = torch.rand((E, size, size), dtype=torch.float64, device=dev) * 360.0
    eng.set_fused(2)

    def host_ms(fn):
        eng.sync()
        t0 = time.perf_counter()
        fn()
        eng.sync()
        return (time.perf_counter() - t0) * 1e3

    for rep in range(REPS + 1):
        # (a)
        eng.reset(xy)
        eng.step(2)                                  # (the cell-major copy exists and is current)
        eng.reset(xy)
        plain = host_ms(lambda: eng.step(2))
        eng.reset(xy)
        res["a_gen"].append(host_ms(lambda: eng.generate_layers(envs, wind_speed=1760.0 + rep, wind_direction=90.0)))
        res["a_rtc"].append(host_ms(lambda: eng.step(2)) - plain)
        # (b), (c)
        eng.set_wind_lab(cache=True, timed=True)
        eng.set_wind(U + rep, D)                     # (fills the cache the first time: generate_layers has staled it)
        eng.set_wind(U + rep + 0.5, D)
        res["b"].append(eng.wind_ms())
        eng.set_wind(fu, fd)
        res["c"].append(eng.wind_ms())
        # (d)
        eng.set_wind_lab(cache=False, timed=True)
        eng.set_wind(U + rep + 0.25, D)
        res["d"].append(eng.wind_ms())
        eng.set_wind_lab(cache=True, timed=True)
        # (e) / (f) with a schedule set and nothing due (its first stepping call builds the first row's tables), then (f) without one
        eng.set_fused(-1)
        eng.set_wind_schedule(None, [(0, 1760.0, 90.0), (1000000, 880.0, 270.0)])
        eng.set_wind_lab(cache=True, timed=False)
        res["f_on"].append(step1_us(eng, xy))
        eng.set_wind_lab(cache=True, timed=True)
        eng.step(1)
        res["e"].append(eng.wind_ms() * 1e3)
        eng.set_wind_schedule(None, [])
        res["f_off"].append(step1_us(eng, xy))
        eng.set_fused(2)
    out = {k: v[1:] for k, v in res.items()}
    out["bytes_written"] = 128 * E * size * ((size + 15) // 16 * 16)
    out["memory_bytes"] = eng.memory_bytes()
    print("RESULT " + json.dumps(out))


def med(v, unit="ms"):
    return "%9.3f [%.3f, %.3f] %s" % (statistics.median(v), min(v), max(v), unit)


def run(args, env=None):
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, capture_output=True, text=True, timeout=1100)
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
    if out.returncode or not line:
        print(out.stdout[-3000:], out.stderr[-3000:])
        raise SystemExit(f"{args} failed ({out.returncode})")
    return json.loads(line[0][7:])


def main():
    if "--child" in sys.argv:
        i = sys.argv.index("--child")
        return (child_parent if sys.argv[i + 1] == "parent" else child)(int(sys.argv[i + 2]), int(sys.argv[i + 3]))
    cases = [(225, 4)] if "--quick" in sys.argv else [(1024, 256), (225, 4)]
    text = (f"Wind change on one MI355X (profiles/wind_probe.py).  Median [min, max] of {REPS} runs after one warm-up run.  (a): host clock around\n"
            "synchronous calls; (b) - (e): GPU time by HIP events around the launches; (f): host clock around 20 synchronous step(1) calls after 21 updates, per call.\n\n")
    for size, E in cases:
        r = run(["--child", "this", str(size), str(E)])
        if os.path.exists(PARENT):
            r.update(run(["--child", "parent", str(size), str(E)], env=dict(os.environ, SIMFIRE_HIP_LIB=PARENT)))
        a = [g + c for g, c in zip(r["a_gen"], r["a_rtc"])]
        text += f"  {size}^2 x {E} (per-environment terrain; the handle holds {r['memory_bytes'] / 2**30:.2f} GiB):\n"
        text += f"    (a) generate_layers, constant wind      {med(r['a_gen'])}   + k_rt_cellmajor at the next resident launch {med(r['a_rtc'])}   = {med(a)}\n"
        text += f"    (b) sf_set_wind uniform, cache warm     {med(r['b'])}   {r['bytes_written'] / statistics.median(r['b']) / 1e6:.0f} GB/s of the 128 B per cell it writes\n"
        text += f"    (c) sf_set_wind device field            {med(r['c'])}\n"
        text += f"    (d) the same kernel from the layers     {med(r['d'])}\n"
        text += f"    (e) schedule pass, nothing due          {med(r['e'], 'us')}\n"
        text += f"    (f) step(1) without a schedule          {med(r['f_off'], 'us')}\n"
        text += f"        step(1) schedule set, nothing due   {med(r['f_on'], 'us')}\n"
        if "f_parent" in r:
            text += f"        step(1) on the parent's library     {med(r['f_parent'], 'us')}\n"
        text += f"    (b) against (a): {statistics.median(a) / statistics.median(r['b']):.1f} times faster (medians); slowest (b) {max(r['b']):.3f} ms, fastest (a) {min(a):.3f} ms\n"
        text += f"    the cache: slowest (b) {max(r['b']):.3f} ms against fastest (d) {min(r['d']):.3f} ms: {'kept' if max(r['b']) < min(r['d']) else 'NOT justified'}\n\n"
    print(text)
    if "--quick" not in sys.argv:
        with open(OUT, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
