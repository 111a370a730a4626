"""Writes tests/golden/atta_worker_mesh.npz: the vertices and triangles of the one scan the reference ships
(fitter_3d/ATTA_BOI/Atta_vollenweideri_1_mg_worker.obj), read with smilify_amd.mesh3d.load_obj (un-normalised).

    python tests/golden/make_mesh3d_fixture.py PATH/TO/Atta_vollenweideri_1_mg_worker.obj
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from smilify_amd.mesh3d import load_obj  # noqa: E402


def main(obj_path):
    v, f = load_obj(obj_path)
    out = os.path.join(HERE, "atta_worker_mesh.npz")
    np.savez_compressed(out, verts=v.numpy().astype(np.float32), faces=f.numpy().astype(np.int32))
    print(out, tuple(v.shape), tuple(f.shape))


if __name__ == "__main__":
    main(sys.argv[1])
