"""Cases of the joined mesh templates beyond tests/mesh_cases.py (include/fdcm.h, "Templates from a mesh: exact visibility and
joined lines"): a ribbon whose boundary is one cycle with two straight borders of 300 edges each, so that the limit of 256
segments per joined line cuts them."""
import numpy as np

import mesh_cases as MC

RIBBON_EDGES, RIBBON_STEP = 300, 1.5


def ribbon(n=RIBBON_EDGES, step=RIBBON_STEP):
    """An open strip in the plane z = 0, n quads of step x 2 step: vertices 2 i at (i step, 0) and 2 i + 1 at (i step, 2 step).
    step = 1.5 is exact in float32 up to i = 300, so under the identity view at scale 1 the borders are exactly collinear edges
    of 1.5 pixels."""
    v = [(i * step, s * 2 * step, 0.0) for i in range(n + 1) for s in (0, 1)]
    f = []
    for i in range(n):
        f += [(2 * i, 2 * i + 2, 2 * i + 3), (2 * i, 2 * i + 3, 2 * i + 1)]
    return np.array(v, dtype=np.float32), np.array(f, dtype=np.int32)


MESHES = dict(MC.MESHES, ribbon=ribbon)
# (name, mesh, views, scale), as MC.CASES
CASES = MC.CASES + [("ribbon", "ribbon", [MC.IDENTITY, MC.GENERIC], 1.0)]
NAMES = [c[0] for c in CASES]


def case(name):
    for n, mesh, views, scale in CASES:
        if n == name:
            v, f = MESHES[mesh]()
            return v, f, np.stack(views), np.float32(scale)
    raise KeyError(name)
