"""The frame spec of ``render`` (tests/_render_oracle.py) against the reference's colour code, Pillow and matplotlib
(tests/golden/render_spec.npz, made by tests/golden/make_golden_render.py), the GIF writer and the save_gif path rules.  No GPU."""
import os
from datetime import datetime
from pathlib import Path

import numpy as np
import pytest

import _render_oracle as ro
from simfire_amd.gif import encode, gif_path, palettize, write_gif
from simfire_amd.render import RenderSpec

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "render_spec.npz"))


def test_dryness_colours_match_pillow_blend():
    alpha = ro.dryness_alpha(GOLD["fuel_w0"], GOLD["fuel_delta"], GOLD["fuel_Mx"])
    assert (alpha < 0).any() and (alpha > 1).any() and ((alpha >= 0) & (alpha <= 1)).any()       # both branches of ImagingBlend
    got = ro.fuel_rgb(GOLD["fuel_w0"], GOLD["fuel_delta"], GOLD["fuel_Mx"], GOLD["texture_rgb"])
    np.testing.assert_array_equal(got, GOLD["fuel_rgb"])


def test_fbfm_colours():
    np.testing.assert_array_equal(ro.fbfm_rgb(GOLD["fbfm_codes"]), GOLD["fbfm_rgb"])
    assert (ro.fbfm_rgb(np.array([0, 14])) == 255).all()          # codes without a colour: white


@pytest.mark.parametrize("i", range(10))
def test_contour_levels_match_matplotlib(i):
    z, lev = GOLD[f"lev_{i}_z"], GOLD[f"lev_{i}_levels"]
    zmin, zmax = float(z.min()), float(z.max())
    inside = [float(L) for L in lev if zmin < L < zmax]
    assert ro.contour_levels(zmin, zmax) == (inside if inside else [zmin])


def test_contour_pixels_rule():
    z = np.array([[0.0, 1.0, 2.0], [1.0, 2.0, 3.0]])
    m = ro.contour_mask(z, [1.0, 2.5])
    # right neighbours: (0,0)-(0,1) crosses 1.0; (1,1)-(1,2) crosses 2.5; lower: (0,0)-(1,0) crosses 1.0, (0,2)-(1,2) crosses 2.5
    np.testing.assert_array_equal(m, [[True, False, True], [False, True, False]])
    assert not ro.contour_mask(np.full((4, 4), 7.0)).any()


def test_downscale_partial_blocks_37x101():
    rng = np.random.default_rng(1)
    status = rng.integers(0, 6, (37, 101))
    fuel = rng.integers(0, 256, (37, 101, 3)).astype(np.uint8)
    cm = rng.uniform(size=(37, 101)) < 0.1
    img, prio = ro.frame(status, fuel, cm)
    for scale in (2, 4):
        for mode in ("nearest", "mean", "sprites"):
            out = ro.downscale(img, prio, scale, mode)
            assert out.shape == (-(-37 // scale), -(-101 // scale), 3)
        mean = ro.downscale(img, prio, scale, "mean")
        last = img[36 // scale * scale:, 100 // scale * scale:].reshape(-1, 3).astype(int)      # the corner block: the cells it has
        np.testing.assert_array_equal(mean[-1, -1], (last.sum(0) + len(last) // 2) // len(last))


def test_sprites_mode_keeps_the_highest_sprite():
    status = np.zeros((4, 4), dtype=np.int64)
    status[0, 0] = 1
    status[1, 1] = 3
    status[2, 2] = 5
    fuel = np.full((4, 4, 3), 100, dtype=np.uint8)
    img, prio = ro.frame(status, fuel, np.zeros((4, 4), bool), agents=[[3, 3, 7]])
    out = ro.downscale(img, prio, 2, "sprites")
    assert tuple(out[0, 0]) == ro.LINE and tuple(out[1, 1]) == ro.AGENT
    out = ro.downscale(img, prio, 4, "sprites")
    assert tuple(out[0, 0]) == ro.AGENT


def test_render_spec_checks():
    s = RenderSpec(4, 37, 101, scale=4)
    assert s.mode == "sprites" and s.shape == (4, 10, 26, 3)
    assert RenderSpec(4, 37, 101, channels_last=False, envs=[1, 1]).shape == (2, 3, 37, 101)
    assert RenderSpec(4, 8, 8, history=(3, 5), envs=[0]).shape == (5, 8, 8, 3)
    for kw in ({"scale": 0}, {"scale": 65}, {"mode": "max"}, {"background": "black"}, {"terrain_rgb": (1, 2, 300)},
               {"envs": [4]}, {"history": (-1, 2)}, {"history": (0, 0)}, {"contours": 1}, {"agents": np.zeros((3, 1, 3))}):
        with pytest.raises(ValueError):
            RenderSpec(4, 8, 8, **kw)


def _decode(path):
    Image = pytest.importorskip("PIL.Image")
    im = Image.open(path)
    out = []
    for i in range(im.n_frames):
        im.seek(i)
        assert im.info.get("loop", 0) == 0
        out += [np.array(im.convert("RGB"))] * (im.info["duration"] // 100)
    return np.stack(out)


@pytest.mark.parametrize("use_pillow", [False, True])
def test_gif_round_trip(tmp_path, use_pillow):
    if use_pillow:
        pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(3)
    pal = rng.integers(0, 256, (40, 3), dtype=np.uint8)
    frames = pal[rng.integers(0, 40, (5, 37, 101))]
    frames[2] = frames[1]
    write_gif(tmp_path / "a.gif", frames, use_pillow=use_pillow)
    np.testing.assert_array_equal(_decode(tmp_path / "a.gif"), frames)


def test_gif_palette_cube_over_256_colours():
    rng = np.random.default_rng(4)
    frames = rng.integers(0, 256, (2, 20, 30, 3), dtype=np.uint8)
    idx, pal = palettize(frames)
    assert np.abs(pal[idx].astype(int) - frames).max() <= 26
    data = encode(frames)
    assert data[:6] == b"GIF89a" and data[-1:] == b";"


def test_gif_literal_encoder_size():
    frames = np.zeros((3, 64, 64, 3), dtype=np.uint8)
    n = encode(frames)
    assert len(n) > 3 * 64 * 64 * 9 // 8          # literal codes: no compression


def test_save_gif_path_rules(tmp_path):
    now = datetime(2026, 1, 2, 3, 4, 5)
    assert gif_path(None, tmp_path, now) == tmp_path / "gifs" / "simulation_2026-01-02_03-04-05.gif"
    assert (tmp_path / "gifs").is_dir()
    assert gif_path(tmp_path / "clips", tmp_path, now) == tmp_path / "clips" / "simulation_2026-01-02_03-04-05.gif"
    assert gif_path(tmp_path / "x" / "run.png", tmp_path, now) == tmp_path / "x" / "run.gif"
    assert (tmp_path / "x").is_dir()
    assert gif_path(str(tmp_path / "y.gif"), tmp_path, now) == tmp_path / "y.gif"
