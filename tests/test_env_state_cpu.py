"""Environment state without a GPU: the blob header as ``SimState`` parses it, its refusals, the C ABI entries the binding declares, and
``copy.deepcopy(FireSimulation)`` refusing a live CFD solver before it touches the device."""
import copy
import os
import re
import struct

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sf_copy_envs", "sf_state_bytes", "sf_save_state", "sf_load_state")


def _header(**over):
    f = dict(magic=0x54534653, version=1, bytes=4096, H=20, W=30, md=4, ab=1, diag=1, att=1, has_max_time=0, prune=0,
             has_parents=0, fire_rows=9, max_time=0.0, update_rate=1.0, pixel_scale=50.0)
    f.update(over)
    raw = struct.pack("<IIq4i4i4i3d", f["magic"], f["version"], f["bytes"], f["H"], f["W"], f["md"], f["ab"], f["diag"], f["att"],
                      f["has_max_time"], f["prune"], f["has_parents"], f["fire_rows"], 0, 0, f["max_time"], f["update_rate"],
                      f["pixel_scale"])
    return raw + bytes(128 - len(raw))


class _FakeEngine:
    """What ``SimState.check`` reads off a FireEngine (no device)."""

    def __init__(self, H=20, W=30, md=4, att=1, nbytes=4096):
        from simfire_amd import _lib
        self.H, self.W = H, W
        self.params = _lib.SfParams(n_envs=2, height=H, width=W, max_fire_duration=md, diagonal_spread=1, attenuate_line_ros=att,
                                    has_max_time=0, pixel_scale=50.0, update_rate=1.0, max_time=0.0)
        self.prune_after_quit = False
        self.spread_graph = False
        self._nb = nbytes

    def state_bytes(self):
        return self._nb


def _state(raw, n=1):
    from simfire_amd.simulation import SimState
    blob = np.zeros((n, 4096), dtype=np.uint8)
    blob[:, :128] = np.frombuffer(raw, dtype=np.uint8)
    return SimState(blob, list(range(n)), np.zeros((n, 2)))


def test_header_parses():
    st = _state(_header(), 2)
    h = st.headers[1]
    assert (h["H"], h["W"], h["max_fire_duration"], h["attenuate_line_ros"], h["fire_rows"]) == (20, 30, 4, True, 9)
    assert len(st) == 2 and not st.on_device
    st.check(_FakeEngine())


@pytest.mark.parametrize("over, engine", [
    (dict(magic=0x12345678), {}),
    (dict(version=2), {}),
])
def test_header_not_a_blob(over, engine):
    with pytest.raises(ValueError):
        _state(_header(**over))


@pytest.mark.parametrize("engine, word", [
    (dict(W=31), "W"),
    (dict(H=21), "H"),
    (dict(md=5), "max_fire_duration"),
    (dict(att=0), "attenuate_line_ros"),
    (dict(nbytes=8192), "bytes"),
])
def test_header_mismatch(engine, word):
    st = _state(_header())
    with pytest.raises(ValueError, match=word):
        st.check(_FakeEngine(**engine))


def test_binding_declares_the_state_entries():
    from simfire_amd import _lib
    header = open(os.path.join(ROOT, "include", "simfire_hip.h")).read()
    for name in NEW:
        assert name in _lib.SIGNATURES
        assert re.search(r"\bint %s\(" % name, header), name
    assert re.search(r"#define SF_COPY_TERRAIN 1\b", header)
    assert len(_lib.SIGNATURES["sf_copy_envs"]) == 5 and len(_lib.SIGNATURES["sf_load_state"]) == 5


def test_deepcopy_refuses_a_cfd_setup():
    from simfire_amd.simulation import FireSimulation

    class _Cfg:
        cfd_setup = object()

    sim = FireSimulation.__new__(FireSimulation)
    sim.config = _Cfg()
    with pytest.raises(TypeError, match="cfd_setup"):
        copy.deepcopy(sim)
