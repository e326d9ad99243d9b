"""Generates ``tests/golden/render_spec.npz`` from the REFERENCE's own colour code and from
real Pillow and matplotlib (a reference checkout, ``SIMFIRE_REFERENCE``; the build machine only).
Run: ``python tests/golden/make_golden_render.py``.

Stored:
- ``texture_rgb``: the reference's terrain texture resized to 1 x 1 (``FunctionalFuelLayer._load_texture``, layers.py:771-784) - the
  base colour the tests pass as ``terrain_rgb`` (nothing derived from the texture is part of the product);
- ``fuel_w0`` / ``fuel_delta`` / ``fuel_Mx`` and ``fuel_rgb``: ``_update_texture_dryness`` (layers.py:744-768, Pillow's
  ``Image.blend``) over a grid of fuel scalars that reaches both of ImagingBlend's branches (alpha inside and outside [0, 1]);
- ``fbfm_codes`` / ``fbfm_rgb``: ``FuelModelRGB13[code] * 255.0`` as ``uint8`` (layers.py:654-667, sprites.py:136-160);
- ``lev_<i>_z`` / ``lev_<i>_levels``: elevation fields and ``ax.contour(z).levels`` (the automatic choice of matplotlib).
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refshim  # noqa: E402,F401

import matplotlib  # noqa: E402
matplotlib.use("Agg")
import matplotlib.pyplot as plt  # noqa: E402
from simfire.enums import FuelModelRGB13  # noqa: E402
from simfire.utils.layers import FunctionalFuelLayer  # noqa: E402


def main():
    out = {}
    texture = FunctionalFuelLayer._load_texture(types.SimpleNamespace())
    out["texture_rgb"] = np.asarray(texture, dtype=np.uint8).reshape(-1)[:3]
    stub = types.SimpleNamespace(texture=texture)
    w0 = np.array([0.0, 0.01, 0.05, 0.1, 0.2296, 0.5, 0.9, 1.0, 1.5, 2.2])
    de = np.array([0.0, 1.0, 3.5, 6.0, 7.0, 14.0])
    mx = np.array([0.0, 0.12, 0.2, 0.5, 0.9, 1.0, 1.8])
    W0, DE, MX = np.meshgrid(w0, de, mx, indexing="ij")
    rgb = np.empty(W0.shape + (3,), dtype=np.uint8)
    for idx in np.ndindex(W0.shape):
        fuel = types.SimpleNamespace(w_0=float(W0[idx]), delta=float(DE[idx]), M_x=float(MX[idx]))
        rgb[idx] = np.asarray(FunctionalFuelLayer._update_texture_dryness(stub, fuel)).reshape(-1)[:3]
    out.update(fuel_w0=W0.ravel(), fuel_delta=DE.ravel(), fuel_Mx=MX.ravel(), fuel_rgb=rgb.reshape(-1, 3))
    codes = np.array(sorted(FuelModelRGB13), dtype=np.int32)
    out["fbfm_codes"] = codes
    out["fbfm_rgb"] = np.stack([(np.asarray(FuelModelRGB13[int(c)]) * 255.0).astype(np.uint8) for c in codes])
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:40, 0:50].astype(np.float64)
    fields = [
        np.full((12, 15), 0.0), np.full((12, 15), 1234.5), np.full((9, 9), -20.0),                                  # flat
        100.0 * np.exp(-((xx - 25) ** 2 + (yy - 20) ** 2) / 200.0),                                                # gaussian hill
        rng.uniform(0, 1, (30, 30)), rng.uniform(-282, 11000, (25, 33)),                                            # noise
        1000.0 + 5.0 * np.sin(xx / 7.0) * np.cos(yy / 5.0),                                                         # large offset
        1.0 + 1e-9 * rng.uniform(0, 1, (10, 10)),                                                                  # tiny range
        3.0 * xx + 0.5 * yy, -50.0 + 0.001 * (xx * yy),
    ]
    for i, z in enumerate(fields):
        fig, ax = plt.subplots()
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            cs = ax.contour(z, origin="upper", colors="black")
        out[f"lev_{i}_z"] = z
        out[f"lev_{i}_levels"] = np.asarray(cs.levels, dtype=np.float64)
        plt.close(fig)
    np.savez_compressed(os.path.join(HERE, "render_spec.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
