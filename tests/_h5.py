"""The h5py the ``data_type: h5`` tests write and read through: the real module where it is installed, else a stand-in
with the part of its API simfire_amd/savedata.py uses - ``File(path, mode)`` as a context manager, ``create_dataset(name,
data=...)`` and ``file[name]`` - that keeps a file's datasets in an .npz container at that path.  With the stand-in the
writer's calls, file names, dtypes and contents are checked all the same; only the bytes on disk are not HDF5."""
import sys
import types

import numpy as np


class _File:
    def __init__(self, path, mode="r"):
        if mode not in ("r", "w"):
            raise ValueError(f"stand-in h5py.File: mode {mode!r} is not used by the writer")
        self.path, self.mode = path, mode
        if mode == "r":
            with np.load(path, allow_pickle=False) as z:
                self.datasets = {k: z[k] for k in z.files}
        else:
            self.datasets = {}

    def create_dataset(self, name, data):
        self.datasets[name] = np.array(data)
        return self.datasets[name]

    def __getitem__(self, name):
        return self.datasets[name]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if self.mode == "w" and exc[0] is None:
            with open(self.path, "wb") as f:
                np.savez(f, **self.datasets)
        return False


def h5py_module(monkeypatch):
    """The real h5py, or the stand-in installed as ``h5py`` for the duration of the test."""
    try:
        import h5py
        return h5py
    except ImportError:
        mod = types.ModuleType("h5py")
        mod.File = _File
        monkeypatch.setitem(sys.modules, "h5py", mod)
        return mod
