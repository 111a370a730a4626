"""Writes tests/golden/rotations_ref.npz: the rotations of the regular and small-angle case sets (tests/rotations_cases.py) through
scipy.spatial.transform.Rotation, an independent statement of the three maps the restatement tests/rotations_ref.py must agree with.

    python tests/golden/make_rotations_fixture.py

Per rotation: ``aa`` the axis-angle input, ``matrix`` = Rotation.from_rotvec(aa).as_matrix(), ``rotvec`` =
Rotation.from_matrix(matrix).as_rotvec() (angle in [0, pi], the branch the standardised quaternion gives).  Half turns are left out:
the sign of their axis is a matter of rounding.  pytorch3d itself cannot be run here, so it is scipy, not pytorch3d, that pins the
restatement.
"""
import os
import sys

import numpy as np
from scipy.spatial.transform import Rotation

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import rotations_cases as CASES  # noqa: E402

N_REGULAR = 200


def main():
    aa = np.concatenate([CASES.regular(N_REGULAR)["aa"].numpy(), CASES.small_angle()["aa"].numpy()])
    matrix = Rotation.from_rotvec(aa).as_matrix()
    rotvec = Rotation.from_matrix(matrix).as_rotvec()
    out = os.path.join(HERE, "rotations_ref.npz")
    np.savez_compressed(out, aa=aa, matrix=matrix, rotvec=rotvec, n_regular=np.int64(N_REGULAR))
    print(f"wrote {out}: {len(aa)} rotations, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
