"""Probe: what values at risk cost (sf_values_set, simfire_amd/csrc/sf_value_kernels.h).

1. The RL tick.  C5's shape (64 x 1024^2, 64 agents per environment), asynchronous mode, one ``sync`` per 100 ticks, random action
   tensors drawn on the device ahead of the timed window; wall time per tick, median [min, max] of 7 windows after one warm-up:

  (a) ``agents_step`` on the library of the commit before this feature (built aside; SIMFIRE_HIP_PARENT names it, default
      profiles/_variants/libsimfire_hip_parent.so; the line is left out where it does not exist),
  (b) this library with everything off,
  (c) arrival recording on,
  (d) arrival + a value plane + the fifth weight,
  (e) (b) with the same loss assembled in torch: ``fire_maps_torch()`` (it waits for the handle's stream and sweeps the blocked plane
      into the row-major one), times the value plane, summed per environment, differenced against the tick before.

   The variants run in child processes of their own (a process loads one build of the library), ROUNDS times in turn, so that the
   repetitions of two variants are interleaved in time.

2. The value pass alone.  C3 (256 x 1024^2) after 5 and after 20 updates from a reset: GPU time by HIP events
   (``time_arrival_pass``) of the arrival pass without a plane, and of the arrival pass + the value pass in its sparse and in its
   dense form; the differences are the value pass.  Each 7 times.

  python profiles/values_probe.py            # -> profiles/values_timing.txt
  python profiles/values_probe.py --quick    # 8 x 256^2, 8 agents, nothing written"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "profiles", "values_timing.txt")
PARENT = os.environ.get("SIMFIRE_HIP_PARENT") or os.path.join(ROOT, "profiles", "_variants", "libsimfire_hip_parent.so")
REPS, TICKS, ROUNDS = 7, 100, 2
WEIGHTS = (-1.0, 0.1, -5.0, -0.1)
NEW = ("sf_values_set", "sf_values_get", "sf_values_device", "sf_values_set_weight", "sf_set_values_dense", "sf_get_value_passes")


def value_plane(H, W):
    """Mostly zero, eight towns of 1 .. 1000."""
    import numpy as np
    rng = np.random.default_rng(20)
    v = np.zeros((H, W), dtype=np.int32)
    for _ in range(8):
        w, h = int(rng.integers(H // 16, H // 4)), int(rng.integers(H // 16, H // 4))
        x, y = int(rng.integers(0, W - w)), int(rng.integers(0, H - h))
        v[y:y + h, x:x + w] = rng.integers(1, 1001, size=(h, w))
    return v


def tick_child(variant, size, E, K):
    import numpy as np
    import torch
    from simfire_amd import _lib, workloads
    if variant == "a":                     # the parent's library does not export the new entry points
        for name in NEW:
            _lib.SIGNATURES.pop(name, None)
    from simfire_amd.engine import FireEngine
    w = workloads.c5(size, E, K)
    dev = "cuda:0"
    eng = FireEngine(**w.engine_kwargs())
    eng.set_layers(*w.layers())
    eng.reset(w.init_xy)
    eng.set_async(True)
    values = value_plane(size, size)
    if variant in "cd":
        eng.enable_arrival(True)
    if variant == "d":
        eng.values_set(values)
    eng.agents_create(K, w.init_xy, n_updates=1, weights=WEIGHTS, only_unburned=True, auto_reset=True)
    rng = np.random.default_rng(9000)
    eng.agents_place(np.arange(E), np.stack([rng.integers(size, size=(E, K)), rng.integers(size, size=(E, K))], axis=2).astype(np.int32))
    if variant == "d":
        eng.agents_set_value_weight(-0.01)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    acts = [torch.randint(0, 20, (E, K), dtype=torch.int32, device=dev, generator=gen) for _ in range(TICKS)]
    o = dict(reward=torch.empty(E, dtype=torch.float32, device=dev), done=torch.empty(E, dtype=torch.uint8, device=dev),
             terms=torch.empty((E, 4), dtype=torch.int32, device=dev), final_len=torch.empty(E, dtype=torch.int32, device=dev),
             final_ret=torch.empty(E, dtype=torch.float64, device=dev))
    vt = torch.from_numpy(values).to(dev).to(torch.int64)
    prev = torch.zeros(E, dtype=torch.int64, device=dev)

    def tick(t):
        nonlocal prev
        eng.agents_step(acts[t % TICKS], **o)
        if variant == "e":
            maps = eng.fire_maps_torch()
            dmg = (((maps == 1) | (maps == 2)) * vt).sum(dim=(1, 2))
            o["reward"] += (-0.01 * (dmg - prev).to(torch.float64)).to(torch.float32)
            prev = dmg
    out = []
    for rep in range(REPS + 1):
        t0 = time.perf_counter()
        for t in range(TICKS):
            tick(rep * TICKS + t)
        eng.sync()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6 / TICKS)
    extra = {}
    if variant == "d":
        extra = dict(passes=eng.value_passes(), damage=int(abs(eng.damage()).sum()))
    print("RESULT " + json.dumps(dict(us=out[1:], **extra)))


def pass_child(size, E):
    from simfire_amd import workloads
    from simfire_amd.engine import FireEngine
    w = workloads.c3(size, E)
    eng = FireEngine(**w.engine_kwargs())
    eng.set_layers(*w.layers())
    eng.reset(w.init_xy)
    eng.enable_arrival(True)
    values = value_plane(size, size)
    res = {}
    for after in (5, 20):
        rows = dict(arrival=[], sparse=[], dense=[])
        for rep in range(REPS + 1):
            eng.values_set(None)
            eng.reset(w.init_xy)
            eng.step(after)
            eng.sync()
            rows["arrival"].append(eng.time_arrival_pass() * 1e3)
            eng.values_set(values)
            eng.set_values_dense(False)
            rows["sparse"].append(eng.time_arrival_pass() * 1e3)
            eng.set_values_dense(True)
            rows["dense"].append(eng.time_arrival_pass() * 1e3)
        res[str(after)] = {k: v[1:] for k, v in rows.items()}
        res[str(after)]["layout"] = eng.cell_layout()
        res[str(after)]["passes"] = eng.value_passes()
    print("RESULT " + json.dumps(res))


def run_child(args, env):
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, capture_output=True, text=True, timeout=900)
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
    if out.returncode or not line:
        print(out.stdout[-2000:], out.stderr[-2000:])
        raise SystemExit(f"{args} failed ({out.returncode})")
    return json.loads(line[0][7:])


def med(v):
    return "%8.1f [%.1f, %.1f]" % (statistics.median(v), min(v), max(v))


def main():
    quick = "--quick" in sys.argv
    size, E, K = (256, 8, 8) if quick else (1024, 64, 64)
    flag = ["--quick"] if quick else []
    if "--tick" in sys.argv:
        return tick_child(sys.argv[sys.argv.index("--tick") + 1], size, E, K)
    if "--pass" in sys.argv:
        return pass_child(size, 8 if quick else 256)
    names = {"a": "the parent commit's library", "b": "this library, everything off", "c": "arrival recording on",
             "d": "arrival + value plane + fifth weight", "e": "(b) + the loss assembled in torch"}
    got = {v: dict(us=[]) for v in names}
    for rnd in range(ROUNDS):
        for v in names:
            env = dict(os.environ)
            if v == "a":
                if not os.path.exists(PARENT):
                    got.pop("a", None)
                    continue
                env["SIMFIRE_HIP_LIB"] = PARENT
            r = run_child(["--tick", v] + flag, env)
            got[v]["us"] += r.pop("us")
            got[v].update(r)
    text = (f"Values at risk on one MI355X.\n\n1. One RL tick: {E} x {size}^2, {K} agents per environment, asynchronous mode, one sync per {TICKS} ticks.  Wall\n"
            f"microseconds per tick, median [min, max] of {ROUNDS} x {REPS} windows of {TICKS} ticks (each round after one warm-up window; the variants take\nturns, a process each).\n\n")
    for v, r in got.items():
        text += f"  ({v}) {names[v]:40s} {med(r['us'])}"
        if "passes" in r:
            text += f"   value passes sparse / dense {r['passes']}, sum of |damage| at the end {r['damage']}"
        text += "\n"
    if "a" in got:
        a, b = got["a"]["us"], got["b"]["us"]
        text += f"\n  (b) against (a): the windows {'overlap' if max(min(a), min(b)) <= min(max(a), max(b)) else 'DO NOT overlap'}\n"
    m = {v: statistics.median(r["us"]) for v, r in got.items()}
    text += f"  (c) - (b) = {m['c'] - m['b']:.1f} us, (d) - (c) = {m['d'] - m['c']:.1f} us, (e) - (b) = {m['e'] - m['b']:.1f} us per tick\n\n"
    p = run_child(["--pass"] + flag, dict(os.environ))
    text += (f"2. The passes alone: {8 if quick else 256} x {size}^2 (C3), GPU microseconds by HIP events of one more pass over the state behind n updates from a\n"
             f"reset, median [min, max] of {REPS}: the arrival pass without a plane, the arrival pass + the value pass (and its commit) in either form.\n\n")
    for after, r in p.items():
        ma, ms, md_ = (statistics.median(r[k]) for k in ("arrival", "sparse", "dense"))
        text += (f"  after {after:>2s} updates (cell layout {r['layout']}):  arrival alone {med(r['arrival'])}   + sparse value pass {med(r['sparse'])}   + dense value pass {med(r['dense'])}\n"
                 f"      the value pass: sparse {ms - ma:.1f} us, dense {md_ - ma:.1f} us\n")
    print(text)
    if not quick:
        with open(OUT, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
