"""What the four queries refuse alike (``sf_distance``, ``sf_reach``, ``sf_walk``, ``sf_behavior``; csrc/sf_host_query.h): the return
code and the WHOLE ``sf_last_error`` text of every shared refusal, which refusal wins when a call has two faults, and that a handle
which refused all of them then answers a good call like the oracle.  Every case is refused on the host before anything is enqueued.

The world is ``_arrival_worlds.make_world("24x40")``: a pitch of 48 bytes, so one environment's scratch is 24 * 48 * 2 = 2304 bytes
for ``sf_distance``, 768 for ``sf_reach`` and 1024 for ``sf_walk`` (two bands of 16 rows x 64 cells).  That world's table comes from
``set_rtable``; ``sf_behavior`` needs layers, so its handle has the world's shape, environments and ignitions over the layers of
``_behavior_worlds.terrain``.  Run with ``pytest -m gpu``."""
import ctypes as C

import numpy as np
import pytest

import _arrival_worlds as aw
import _behavior_worlds as bw
import test_behavior_gpu as tb
import test_distance_gpu as td
import test_reach_gpu as tr
import test_walk_gpu as tw

pytestmark = pytest.mark.gpu
BURNING, UNBURNED = ("BURNING",), ("UNBURNED",)
OK, EINVAL, ESTATE = "SF_OK", "SF_EINVAL", "SF_ESTATE"

PARAMS = dict(distance="SfDistParams", reach="SfReachParams", walk="SfWalkParams", behavior="SfBehaviorParams")
OUTS = dict(reach="SfReachOut", walk="SfWalkOut", behavior="SfBehaviorOut")
#: a valid call: these fields, every environment in order, this one output (at BUF)
VALID = dict(distance=dict(status_mask=2, scale=1.0), reach=dict(source_mask=2, through_mask=1), walk=dict(target_mask=2, through_mask=1),
             behavior=dict(status_mask=0, summary_mask=2))
FIRST_OUT = dict(distance="out", reach="count", walk="reached", behavior="max_flame")

# Table one: per call one bad call per shared refusal - (what differs from the valid call, code, text).  "BUF" / "PTS": the address
# of the output buffer / of a points tensor [E, 3, 3], "+ n": n bytes on.
ONE = {
    "distance": [
        (dict(k=257, points="PTS"), EINVAL, "sf_distance: 257 points per environment (0..256)"),
        (dict(k=-1), EINVAL, "sf_distance: -1 points per environment (0..256)"),
        (dict(k=3), EINVAL, "sf_distance: k = 3 needs points"),
        (dict(scratch_bytes=2303), EINVAL, "sf_distance: scratch_bytes 2303 is less than one environment's plane (2304 bytes)"),
        (dict(reserved=1), EINVAL, "sf_distance: reserved must be 0"),
        (dict(outs=dict(out="BUF+2")), EINVAL, "sf_distance: the output is not aligned to its element"),
        (dict(envs=[0, 99]), EINVAL, "sf_distance: environment 99 out of range"),
    ],
    "reach": [
        (dict(k=257, points="PTS"), EINVAL, "sf_reach: 257 points per environment (0..256)"),
        (dict(k=-1), EINVAL, "sf_reach: -1 points per environment (0..256)"),
        (dict(k=3), EINVAL, "sf_reach: k = 3 needs points"),
        (dict(scratch_bytes=767), EINVAL, "sf_reach: scratch_bytes 767 is less than one environment's need (768 bytes)"),
        (dict(reserved=1), EINVAL, "sf_reach: reserved must be 0"),
        (dict(outs=dict(count="BUF+2")), EINVAL, "sf_reach: an output is not aligned to its element"),
        (dict(outs=dict(value="BUF+4")), EINVAL, "sf_reach: an output is not aligned to its element"),
        (dict(envs=[0, 99]), EINVAL, "sf_reach: environment 99 out of range"),
    ],
    "walk": [
        (dict(k=257, points="PTS"), EINVAL, "sf_walk: 257 points per environment (0..256)"),
        (dict(k=-1), EINVAL, "sf_walk: -1 points per environment (0..256)"),
        (dict(k=3), EINVAL, "sf_walk: k = 3 needs points"),
        (dict(points="PTS"), EINVAL, "sf_walk: points need k > 0"),
        (dict(scratch_bytes=1023), EINVAL, "sf_walk: scratch_bytes 1023 is less than one environment's need (1024 bytes)"),
        (dict(reserved=1), EINVAL, "sf_walk: reserved must be 0"),
        (dict(outs=dict(reached="BUF+2")), EINVAL, "sf_walk: an output is not aligned to its element"),
        (dict(envs=[0, 99]), EINVAL, "sf_walk: environment 99 out of range"),
    ],
    "behavior": [                 # (no scratch)
        (dict(k=257, points="PTS", outs=dict(point_flame="BUF")), EINVAL, "sf_behavior: 257 points per environment (0..256)"),
        (dict(k=-1), EINVAL, "sf_behavior: -1 points per environment (0..256)"),
        (dict(k=3, outs=dict(point_flame="BUF")), EINVAL, "sf_behavior: k = 3 needs points"),
        (dict(points="PTS"), EINVAL, "sf_behavior: points need k > 0"),
        (dict(reserved=1), EINVAL, "sf_behavior: reserved must be 0"),
        (dict(outs=dict(max_flame="BUF+2")), EINVAL, "sf_behavior: an output is not aligned to its element"),
        (dict(envs=[0, 99]), EINVAL, "sf_behavior: environment 99 out of range"),
    ],
}

# Table two: calls with two faults (or a valid call on a handle that is not ready), and the refusal that wins: arguments in the order
# of the entry's checks, then the environment list, then what the handle lacks (SF_ESTATE: check_ready before the feature's own),
# and only then "a list of none is SF_OK".
TWO = {
    "distance": {
        "before reset": [
            (dict(status_mask=0), EINVAL, "sf_distance: status_mask 0 (bit s selects BurnStatus s: 1..63)"),
            (dict(envs=[99]), EINVAL, "sf_distance: environment 99 out of range"),
            (dict(), ESTATE, "sf_distance: call sf_reset first"),
            (dict(n=0), ESTATE, "sf_distance: call sf_reset first"),
        ],
        "after reset": [
            (dict(k=257, points="PTS", outs=dict(out="BUF+2")), EINVAL, "sf_distance: 257 points per environment (0..256)"),
            (dict(k=3, reserved=1), EINVAL, "sf_distance: k = 3 needs points"),
            (dict(reserved=1, envs=[99]), EINVAL, "sf_distance: reserved must be 0"),
            (dict(outs=dict(out="BUF+2"), scratch_bytes=1), EINVAL, "sf_distance: the output is not aligned to its element"),
            (dict(scratch_bytes=1, envs=[99]), EINVAL, "sf_distance: scratch_bytes 1 is less than one environment's plane (2304 bytes)"),
        ],
    },
    "reach": {
        "before reset": [
            (dict(source_mask=0), EINVAL, "sf_reach: source_mask 0 (bit s selects BurnStatus s: 1..63)"),
            (dict(envs=[99]), EINVAL, "sf_reach: environment 99 out of range"),
            (dict(), ESTATE, "sf_reach: call sf_reset first"),
            (dict(outs=dict(value="BUF")), ESTATE, "sf_reach: call sf_reset first"),
        ],
        "after reset": [
            (dict(k=257, points="PTS", outs=dict(count="BUF+2")), EINVAL, "sf_reach: 257 points per environment (0..256)"),
            (dict(reserved=1, outs=dict(count="BUF+2")), EINVAL, "sf_reach: reserved must be 0"),
            (dict(outs=dict(count="BUF+2"), scratch_bytes=-1), EINVAL, "sf_reach: an output is not aligned to its element"),
            (dict(scratch_bytes=-1, envs=[99]), EINVAL, "sf_reach: scratch_bytes -1 is less than one environment's need (768 bytes)"),
            (dict(outs=dict(value="BUF"), envs=[99]), EINVAL, "sf_reach: environment 99 out of range"),
            (dict(outs=dict(value="BUF")), ESTATE, "sf_reach: value needs a value plane (sf_values_set)"),
            (dict(outs=dict(value="BUF"), n=0), ESTATE, "sf_reach: value needs a value plane (sf_values_set)"),
        ],
    },
    "walk": {
        "before reset": [
            (dict(through_mask=0), EINVAL, "sf_walk: through_mask 0 (bit s selects BurnStatus s: 1..63)"),
            (dict(envs=[99]), EINVAL, "sf_walk: environment 99 out of range"),
            (dict(), ESTATE, "sf_walk: call sf_reset first"),
        ],
        "after reset": [
            (dict(k=257, points="PTS", outs=dict(reached="BUF+2")), EINVAL, "sf_walk: 257 points per environment (0..256)"),
            (dict(points="PTS", reserved=1), EINVAL, "sf_walk: points need k > 0"),
            (dict(reserved=1, outs=dict(reached="BUF+2")), EINVAL, "sf_walk: reserved must be 0"),
            (dict(scratch_bytes=-1, envs=[99]), EINVAL, "sf_walk: scratch_bytes -1 is less than one environment's need (1024 bytes)"),
        ],
    },
    "behavior": {
        "before reset": [
            (dict(summary_mask=0), EINVAL, "sf_behavior: summary_mask 0 (bit s selects BurnStatus s: 1..63)"),
            (dict(envs=[99]), EINVAL, "sf_behavior: environment 99 out of range"),
            (dict(), ESTATE, "sf_behavior: call sf_reset first"),
        ],
        "after reset": [
            (dict(reserved=1, k=257), EINVAL, "sf_behavior: reserved must be 0"),
            (dict(k=257, envs=[99]), EINVAL, "sf_behavior: 257 points per environment (0..256)"),
            (dict(outs=dict(max_flame="BUF+2"), envs=[99]), EINVAL, "sf_behavior: an output is not aligned to its element"),
        ],
    },
}

# sf_behavior on the world's own handle, whose table came from set_rtable: the feature's own SF_ESTATE, behind check_ready's
NO_LAYERS = {
    "before reset": [(dict(), ESTATE, "sf_behavior: call sf_reset first")],
    "after reset": [
        (dict(reserved=1), EINVAL, "sf_behavior: reserved must be 0"),
        (dict(envs=[99]), EINVAL, "sf_behavior: environment 99 out of range"),
        (dict(), ESTATE, "sf_behavior: environment 0's table came from sf_set_rtable: there are no layers to take the reaction intensity from"),
        (dict(envs=[2, 1]), ESTATE, "sf_behavior: environment 2's table came from sf_set_rtable: there are no layers to take the reaction intensity from"),
        (dict(n=0), OK, None),
    ],
}


def _raw(q, eng, buf, pts):
    """rc(**what differs from the valid call) -> (the code's name, the text of ``sf_last_error``) of the raw call ``sf_<q>``.
    ``n``, ``envs``, ``reserved`` (the first reserved word), ``outs`` (name -> address; sf_distance: ``out``), else a field."""
    from simfire_amd import _lib
    names = {getattr(_lib, c): c for c in ("SF_OK", "SF_EINVAL", "SF_ESTATE", "SF_ENOTSUP", "SF_EHIP")}
    where = {"BUF": buf.data_ptr(), "PTS": pts.data_ptr()}

    def address(v):
        if isinstance(v, dict):
            return {k: address(x) for k, x in v.items()}
        if isinstance(v, str):
            base, _, off = v.partition("+")
            return where[base] + int(off or 0)
        return v

    def rc(n=None, envs=None, reserved=0, outs=None, **fields):
        envs = np.arange(eng.n_envs, dtype=np.int32) if envs is None else np.ascontiguousarray(envs, dtype=np.int32)
        n = len(envs) if n is None else n
        p = getattr(_lib, PARAMS[q])(**address(dict(VALID[q], **fields)))
        if q == "behavior":
            p.reserved = reserved
            for i, v in enumerate((4.0, 8.0, 11.0, 1e30)):
                p.edges[i] = v
        else:
            p.reserved[0] = reserved
        outs = address({FIRST_OUT[q]: "BUF"} if outs is None else outs)
        ep = envs.ctypes.data_as(C.c_void_p)
        if q == "distance":
            code = eng._L.sf_distance(eng._h, C.byref(p), n, ep, C.c_void_p(outs["out"]))
        elif q == "behavior":
            code = eng._L.sf_behavior(eng._h, C.byref(p), C.byref(_lib.SfBehaviorOut(**outs)), ep, n)
        else:
            code = getattr(eng._L, "sf_" + q)(eng._h, C.byref(p), n, ep, C.byref(getattr(_lib, OUTS[q])(**outs)))
        return names[code], eng._L.sf_last_error().decode() if code else None
    return rc


def _table(q, rc, rows):
    for kwargs, code, text in rows:
        got = rc(**kwargs)
        print(q, kwargs, "->", got)
        assert got == (code, text), (q, kwargs, got, (code, text))


def _buffers(E, H, W):
    import torch
    return (torch.full((E * H * W,), -7, dtype=torch.int32, device="cuda"), torch.zeros((E, 3, 3), dtype=torch.int32, device="cuda"))


@pytest.mark.parametrize("q", list(ONE))
def test_refusals_then_a_good_call(q):
    kw, R8, E, inits = aw.make_world("24x40")
    H, W = kw["shape"]
    if q == "behavior":
        layers = bw.terrain(2561, H, W, E)
        eng = bw.engine(H, W, layers, mode="run")
    else:
        eng = tw._engine(kw, E, R8, "run")
    buf, pts = _buffers(E, H, W)
    rc = _raw(q, eng, buf, pts)
    _table(q, rc, TWO[q]["before reset"])
    eng.reset(inits)
    eng.step(3)
    held = eng.memory_bytes()
    _table(q, rc, ONE[q])
    _table(q, rc, TWO[q]["after reset"])
    eng.sync()
    assert bool((buf == -7).all()) and eng.memory_bytes() == held      # nothing was enqueued, no scratch was made
    if q == "behavior":
        assert eng.behavior_builds() == 0

    # the handle answers as if nothing had been refused
    assert rc(n=0) == (OK, None)
    if q in ("distance", "reach"):
        assert rc(points="PTS") == (OK, None)              # (these two ignore points that come with k == 0)
    if q == "distance":
        got, want, _ = td._planes(eng, BURNING)
        td._same(got, want, "after the refusals")
    elif q == "reach":
        r, maps, _ = tr._ask(eng, BURNING, UNBURNED, 0)
        tr._same(r, maps, range(E), BURNING, UNBURNED, tr._conn(kw, 0), "after the refusals")
    elif q == "walk":
        r, maps, _ = tw._ask(eng, BURNING, UNBURNED, 4)
        tw._same(r, maps, range(E), BURNING, UNBURNED, 4, "after the refusals")
    else:
        r, _ = tb._ask(eng)
        tb._check(eng, r, None, lambda e: layers[e], tag="after the refusals")
    eng.close()


def test_behavior_refuses_a_table_without_layers():
    kw, R8, E, inits = aw.make_world("24x40")
    H, W = kw["shape"]
    eng = tw._engine(kw, E, R8, "run")
    buf, pts = _buffers(E, H, W)
    rc = _raw("behavior", eng, buf, pts)
    _table("behavior", rc, NO_LAYERS["before reset"])
    eng.reset(inits)
    eng.step(3)
    held = eng.memory_bytes()
    _table("behavior", rc, NO_LAYERS["after reset"])
    eng.sync()
    assert bool((buf == -7).all()) and eng.memory_bytes() == held and eng.behavior_builds() == 0
    eng.close()
