"""Animated GIFs of recorded frames (``FireSimulation.save_gif``), without a dependency on Pillow.

The palette is exact when a clip has at most 256 colours (the frames of ``render`` usually do: terrain shades, contours and six
sprite colours); otherwise every colour is mapped into a fixed 6 x 7 x 6 cube.  The encoder writes "uncompressed" LZW: every pixel
is a 9-bit literal code, with a clear code often enough that the code width never grows - NumPy-vectorised, about 9/8 bytes per
pixel.  Where Pillow is importable it writes the same palette images with real LZW compression instead, for smaller files.
"""
from datetime import datetime
from pathlib import Path
from typing import Optional, Union

import numpy as np

_CUBE = (6, 7, 6)
_RUN = 250            # literal codes between two clear codes: the decoder's table stays below 512 entries (9-bit codes throughout)


def gif_path(path: Optional[Union[str, Path]], sf_home: Path, now: Optional[datetime] = None) -> Path:
    """The file ``save_gif(path)`` writes (simfire/sim/simulation.py:831-860): default ``<sf_home>/gifs/simulation_<now>.gif``; a
    suffix-less path is a directory that gets that file name; any other suffix is replaced by ``.gif``.  Parents are created."""
    path = Path(sf_home) / "gifs" if path is None else Path(path).expanduser()
    if path.suffix == "":
        stamp = (now or datetime.now()).strftime("%Y-%m-%d_%H-%M-%S")
        path = path / f"simulation_{stamp}.gif"
    path.parent.mkdir(parents=True, exist_ok=True)
    if path.suffix != ".gif":
        path = path.with_suffix(".gif")
    return path


def palettize(frames: np.ndarray):
    """uint8 [k, H, W, 3] -> (indices uint8 [k, H, W], palette uint8 [256, 3]): exact with at most 256 distinct colours, else the
    6 x 7 x 6 cube (each channel to its nearest cube level)."""
    f = np.ascontiguousarray(frames, dtype=np.uint8)
    packed = f[..., 0].astype(np.uint32) | f[..., 1].astype(np.uint32) << 8 | f[..., 2].astype(np.uint32) << 16
    colours = np.unique(packed)
    palette = np.zeros((256, 3), dtype=np.uint8)
    if colours.size <= 256:
        idx = np.searchsorted(colours, packed).astype(np.uint8)
        palette[:colours.size, 0] = colours & 0xFF
        palette[:colours.size, 1] = (colours >> 8) & 0xFF
        palette[:colours.size, 2] = colours >> 16
        return idx, palette
    lv = [np.rint(np.arange(n) * 255.0 / (n - 1)).astype(np.uint8) for n in _CUBE]
    q = [np.rint(f[..., c].astype(np.float64) * (_CUBE[c] - 1) / 255.0).astype(np.int64) for c in range(3)]
    idx = (q[0] * (_CUBE[1] * _CUBE[2]) + q[1] * _CUBE[2] + q[2]).astype(np.uint8)
    r, g, b = np.meshgrid(lv[0], lv[1], lv[2], indexing="ij")
    n = int(np.prod(_CUBE))
    palette[:n] = np.stack([r.ravel(), g.ravel(), b.ravel()], axis=1)
    return idx, palette


def _lzw_literal(idx: np.ndarray) -> bytes:
    """Image data of one frame: minimum code size 8, then 9-bit codes [clear, up to _RUN literals]..., end; in sub-blocks."""
    px = idx.reshape(-1).astype(np.uint16)
    n = px.size
    runs = -(-n // _RUN)
    codes = np.empty(n + runs + 1, dtype=np.uint16)
    pos = np.arange(n) + np.arange(n) // _RUN + 1          # each run is preceded by its clear code
    codes[pos] = px
    codes[np.arange(runs) * (_RUN + 1)] = 256
    codes[-1] = 257
    bits = ((codes[:, None] >> np.arange(9, dtype=np.uint16)) & 1).astype(np.uint8).reshape(-1)
    data = np.packbits(bits, bitorder="little")
    full, rest = divmod(data.size, 255)
    blocks = np.empty(full * 256 + (rest + 1 if rest else 0), dtype=np.uint8)
    head = blocks[:full * 256].reshape(full, 256)
    head[:, 0] = 255
    head[:, 1:] = data[:full * 255].reshape(full, 255)
    if rest:
        blocks[full * 256] = rest
        blocks[full * 256 + 1:] = data[full * 255:]
    return b"\x08" + blocks.tobytes() + b"\x00"


def encode(frames: np.ndarray, duration: int = 100, loop: int = 0) -> bytes:
    """GIF89a bytes of uint8 frames [k, H, W, 3] with the encoder of this module (no Pillow)."""
    idx, palette = palettize(frames)
    k, H, W = idx.shape
    out = [b"GIF89a", np.array([W, H], dtype="<u2").tobytes(), bytes([0xF7, 0, 0]), palette.tobytes(),
           b"\x21\xFF\x0BNETSCAPE2.0\x03\x01" + np.array([loop], dtype="<u2").tobytes() + b"\x00"]
    delay = np.array([int(round(duration / 10))], dtype="<u2").tobytes()
    for i in range(k):
        out.append(b"\x21\xF9\x04\x00" + delay + b"\x00\x00")
        out.append(b"\x2C" + np.array([0, 0, W, H], dtype="<u2").tobytes() + b"\x00")
        out.append(_lzw_literal(idx[i]))
    out.append(b"\x3B")
    return b"".join(out)


def write_gif(path: Union[str, Path], frames: np.ndarray, duration: int = 100, loop: int = 0, use_pillow: Optional[bool] = None) -> None:
    """Write frames [k, H, W, 3] as an animated GIF (``duration`` ms per frame, ``loop`` 0 = for ever, as game.py:295-315 does).
    ``use_pillow``: None = when importable.  Pillow merges a frame identical to the one before into it (their durations add up)."""
    frames = np.asarray(frames)
    if frames.ndim != 4 or frames.shape[-1] != 3 or frames.shape[0] == 0:
        raise ValueError(f"frames must be [k >= 1, H, W, 3], got {frames.shape}")
    if use_pillow is None:
        try:
            import PIL.Image  # noqa: F401
            use_pillow = True
        except ImportError:
            use_pillow = False
    if not use_pillow:
        Path(path).write_bytes(encode(frames, duration, loop))
        return
    from PIL import Image
    idx, palette = palettize(frames)
    ims = []
    for i in range(idx.shape[0]):
        im = Image.frombytes("P", (idx.shape[2], idx.shape[1]), np.ascontiguousarray(idx[i]).tobytes())
        im.putpalette(palette.reshape(-1).tolist())
        ims.append(im)
    ims[0].save(path, format="GIF", save_all=True, append_images=ims[1:], duration=duration, loop=loop, optimize=False)
