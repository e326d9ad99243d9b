"""Probe: what one RL tick costs with the agents on the device (sf_agents_step, simfire_amd/csrc/sf_agent_kernels.h).

C5's shape (64 x 1024^2, 64 agents per environment, attenuation on), asynchronous mode, one ``sync`` per 100 ticks, random
action tensors drawn on the device ahead of the timed window:

  (a) ``FireEngine.agents_step`` with all five outputs (auto_reset on, only_unburned on),
  (b) the same tick assembled from what the library offered before: torch ops turn the action tensor into moves, the cell under
      each agent (a gather from ``fire_maps_torch``'s plane, refreshed before and after the update: each refresh waits for the
      handle's stream and converts the whole plane, so (b) waits on the host twice per tick), the points and the counts; ``step_mitigated``
      takes the points as a device tensor; ``rollout`` leaves the result block in a sink tensor; torch differences the block into
      reward / done and re-places the agents; ``reset_where`` restarts the done environments from the device mask.
  (c) for scale: the one-update ``step_mitigated`` call alone, with constant points.

Wall time per tick: host clock around 100 ticks and the sync, divided by 100; median [min, max] of 7 windows after one warm-up.
Nothing is gated on these numbers.

  python profiles/agents_step_probe.py            # -> profiles/agents_step_timing.txt
  python profiles/agents_step_probe.py --quick    # 8 x 256^2, 8 agents, nothing written"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from simfire_amd import workloads  # noqa: E402
from simfire_amd.engine import FireEngine  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "agents_step_timing.txt")
REPS, TICKS = 7, 100
WEIGHTS = (-1.0, 0.1, -5.0, -0.1)


def engine(w):
    eng = FireEngine(**w.engine_kwargs())
    eng.set_layers(*w.layers())
    eng.reset(w.init_xy)
    eng.set_async(True)
    return eng


def starts(E, K, H, W):
    rng = np.random.default_rng(9000)
    return np.stack([rng.integers(W, size=(E, K)), rng.integers(H, size=(E, K))], axis=2).astype(np.int32)


def windows(tick, eng):
    out = []
    for rep in range(REPS + 1):
        t0 = time.perf_counter()
        for t in range(TICKS):
            tick(rep * TICKS + t)
        eng.sync()
        out.append((time.perf_counter() - t0) * 1e6 / TICKS)
    return out[1:]


def probe(size, E, K):
    import torch
    w = workloads.c5(size, E, K)
    H = W = size
    dev = "cuda:0"
    xy0 = starts(E, K, H, W)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    acts = [torch.randint(0, 20, (E, K), dtype=torch.int32, device=dev, generator=gen) for _ in range(TICKS)]
    ign = torch.from_numpy(np.ascontiguousarray(w.init_xy, dtype=np.int32)).to(dev)

    # (a) the device tick
    eng = engine(w)
    eng.agents_create(K, w.init_xy, n_updates=1, weights=WEIGHTS, only_unburned=True, auto_reset=True)
    eng.agents_place(np.arange(E), xy0)
    o = dict(reward=torch.empty(E, dtype=torch.float32, device=dev), done=torch.empty(E, dtype=torch.uint8, device=dev),
             terms=torch.empty((E, 4), dtype=torch.int32, device=dev), final_len=torch.empty(E, dtype=torch.int32, device=dev),
             final_ret=torch.empty(E, dtype=torch.float64, device=dev))
    a = windows(lambda t: eng.agents_step(acts[t % TICKS], **o), eng)
    eng.close()

    # (b) the torch assembly on the calls that existed before
    eng = engine(w)
    pos = torch.from_numpy(xy0).to(dev).to(torch.int64)
    start = pos.clone()
    sink = torch.zeros((E, 8), dtype=torch.int32, device=dev)
    eng.set_result_sink(sink.data_ptr())
    eng.rollout(0, sink.data_ptr())
    eng.sync()
    ep_len = torch.zeros(E, dtype=torch.int32, device=dev)
    ep_ret = torch.zeros(E, dtype=torch.float64, device=dev)
    wt = torch.tensor(WEIGHTS, dtype=torch.float64, device=dev)
    env_ix = torch.arange(E, device=dev)[:, None].expand(E, K)
    dx = torch.tensor([0, 0, 0, -1, 1], device=dev)
    dy = torch.tensor([0, -1, 1, 0, 0], device=dev)

    def assembled(t):
        nonlocal pos, ep_len, ep_ret
        act = acts[t % TICKS].to(torch.int64)
        act = torch.where((act < 0) | (act > 19), torch.zeros_like(act), act)
        running = sink[:, 0] == 1
        prev = (sink[:, 3] + sink[:, 4]).clone()
        move, inter = act % 5, act // 5
        nx, ny = pos[..., 0] + dx[move], pos[..., 1] + dy[move]
        ok = (nx >= 0) & (nx < W) & (ny >= 0) & (ny < H)
        live = running[:, None]
        blocked = (~ok & live).sum(1)
        x = torch.where(ok & live, nx, pos[..., 0])
        y = torch.where(ok & live, ny, pos[..., 1])
        maps = eng.fire_maps_torch()
        emit = (inter > 0) & live & (maps[env_ix, y, x] == 0)
        pts = torch.stack([x, y, torch.where(emit, inter + 2, torch.zeros_like(inter))], dim=2).to(torch.int32)[None].contiguous()
        eng.step_mitigated(pts)
        eng.rollout(0, sink.data_ptr())
        maps = eng.fire_maps_torch()
        in_fire = ((maps[env_ix, y, x] == 1) & live).sum(1)
        terms = torch.stack([(sink[:, 3] + sink[:, 4]) - prev, emit.sum(1), in_fire, blocked], dim=1).to(torch.float64)
        reward = torch.where(running, (terms * wt).sum(1), torch.zeros(E, dtype=torch.float64, device=dev)).to(torch.float32)
        ep_len = ep_len + running.to(torch.int32)
        ep_ret = ep_ret + reward.to(torch.float64)
        done = ~running | (sink[:, 0] != 1)
        eng.reset_where(done.to(torch.uint8), ign)
        pos = torch.where(done[:, None, None], start, torch.stack([x, y], dim=2))
        ep_len = torch.where(done, torch.zeros_like(ep_len), ep_len)
        ep_ret = torch.where(done, torch.zeros_like(ep_ret), ep_ret)

    b = windows(assembled, eng)
    eng.set_result_sink(None)
    eng.close()

    # (c) the one-update step_mitigated call alone
    eng = engine(w)
    pts = torch.zeros((1, E, K, 3), dtype=torch.int32, device=dev)
    pts[0, :, :, :2] = torch.from_numpy(xy0).to(dev)
    pts[0, :, :, 2] = 3
    c = windows(lambda t: eng.step_mitigated(pts), eng)
    eng.close()
    return a, b, c


def med(v):
    return "%8.1f us  [%.1f, %.1f]" % (statistics.median(v), min(v), max(v))


def main():
    quick = "--quick" in sys.argv
    size, E, K = (256, 8, 8) if quick else (1024, 64, 64)
    a, b, c = probe(size, E, K)
    ratio = statistics.median(b) / statistics.median(a)
    shape = "" if quick else " (C5's shape)"
    text = (f"One RL tick on one MI355X: {E} x {size}^2, {K} agents per environment{shape}, asynchronous mode, one sync per {TICKS} ticks.\n"
            f"Wall time per tick, median [min, max] of {REPS} windows of {TICKS} ticks after one warm-up window.\n\n"
            f"  (a) agents_step (sf_agents_step, all outputs, auto_reset)          {med(a)}\n"
            f"  (b) the same tick from torch ops + step_mitigated + rollout\n"
            f"      into a sink + reset_where                                       {med(b)}\n"
            f"  (c) step_mitigated(one update, device points) alone                 {med(c)}\n\n"
            f"  (b) / (a) = {ratio:.2f}\n"
            f"  (a) - (c) = {statistics.median(a) - statistics.median(c):.1f} us.  The expectation was (c) plus two wave-sized launches (a few us each).  The tick\n"
            f"  also enqueues the two launches of the batched reset (auto_reset) and, where the step ran as per-step launches, a count of the\n"
            f"  result block; and the Python binding checks six tensors and waits for torch's queued work before every call, which (c) does not.\n"
            f"  (b) is not only the dozen small torch launches: the cell under each agent comes from fire_maps_torch(), which waits for the\n"
            f"  handle's stream and sweeps the whole blocked plane into the row-major one, twice per tick - the older calls offer no cheaper\n"
            f"  way to read single cells on the device.  Most of (b) / (a) is those two waits and sweeps.\n"
            + ("  The device tick is SLOWER than the torch assembly.\n" if ratio < 1.0 else ""))
    print(text)
    if not quick:
        with open(OUT, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
