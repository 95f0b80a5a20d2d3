#!/usr/bin/env python3
"""Generate tests/golden/sid_tables.npz by RUNNING THE REFERENCE's ``get_depth_sid`` and ``get_labels_sid`` (utils.py:120-193) on the CPU, for its
four parameter sets.  Only inputs that are re-derivable and the functions' OUTPUTS are stored, per name N:
  N/depth_of_label   (K+1,) float32   get_depth_sid(N, torch.arange(K + 1))
  N/grid             (K+3,) float32   depths: the float64 bin centres alpha * (beta / alpha) ** ((k + 0.5) / K), k = 0..K-1, rounded to float32 -
                                      half a label away from every truncation boundary of ``.int()`` - then beta / 2, beta * 0.9 and beta * 2
  N/label_of_grid    (K+3,) int32     get_labels_sid(N, grid)
  N/params           (3,)   float64   alpha, beta, K as the reference's branches state them (settings, not code)
``utils.py`` imports plotting and loader modules it does not need for these two functions; whichever of them is missing where this runs is
replaced by a stand-in in ``sys.modules`` for the import.

Usage:  python tests/golden/make_sid_golden.py REFERENCE_DIR        (regenerates the file bit for bit)
"""
import os
import sys
import types
from unittest import mock

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))

import numpy as np
import torch

PARAMS = {"nyu": (0.02, 10.0, 90.0), "kitti": (0.001, 80.0, 71.0), "floorplan3d": (0.0552, 10.0, 68.0), "Structured3D": (0.02, 10.0, 68.0)}


def import_reference_utils(ref):
    sys.path.insert(0, ref)
    for _ in range(32):
        try:
            import utils as u
            return u
        except ImportError as e:                                      # a module utils.py names but these functions never touch
            if not e.name or e.name == "utils":
                raise
            parts = e.name.split(".")
            for i in range(1, len(parts) + 1):
                sys.modules.setdefault(".".join(parts[:i]), mock.MagicMock(spec=types.ModuleType, name=".".join(parts[:i])))
    raise ImportError("utils.py of the reference does not import")


def grid(alpha, beta, K):
    k = np.arange(int(K), dtype=np.float64) + 0.5
    g = alpha * (beta / alpha) ** (k / K)
    return np.concatenate([g, [beta / 2.0, beta * 0.9, beta * 2.0]]).astype(np.float32)


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    u = import_reference_utils(sys.argv[1])
    out = {}
    for name, (alpha, beta, K) in PARAMS.items():
        labels = torch.arange(int(K) + 1)
        d = u.get_depth_sid(name, labels)
        g = grid(alpha, beta, K)
        lab = u.get_labels_sid(name, torch.from_numpy(g))
        assert d.dtype == torch.float32 and lab.dtype == torch.int32
        assert abs(float(d[0]) - alpha) < 1e-6 * alpha and abs(float(d[-1]) - beta) < 1e-5 * beta, (name, d[0], d[-1])   # the table above matches the branches
        assert (lab[:int(K)].numpy() == np.arange(int(K))).all(), name
        out[name + "/depth_of_label"] = d.numpy()
        out[name + "/grid"] = g
        out[name + "/label_of_grid"] = lab.numpy()
        out[name + "/params"] = np.array([alpha, beta, K], dtype=np.float64)
    np.savez(os.path.join(HERE, "sid_tables.npz"), **out)
    print("wrote sid_tables.npz:", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
