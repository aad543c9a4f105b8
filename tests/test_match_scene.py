"""CPU-only: the end-to-end scene of the calls on match lists (tests/match_scene.py) gives what test_gpu_matches.py asks of the
device.  On the oracle's match list the referee (tests/match_ref.py) keeps exactly two records at MAX_SCORE, one per
instance of the part, and MAX_SCORE lies between the q of the records on the instances and the best junk's."""
import numpy as np

import match_ref as R
import match_scene as MS
from oracle import oracle as O


def test_the_scene_gives_one_record_per_instance():
    scene, tmpls, centres = MS.two_parts()
    orc = O.build(scene, depth=30, coeff=5.0, padding=2.2, distance=O.L2, nthreads=2)
    raw = O.search(orc, tmpls, scene, MS.MAX_TMPL, MS.MAX_SCENE, kind=O.BATCH_OPTIMIZE, batch=10, nthreads=2)
    den = R.denominators(tmpls, 0)
    q = raw["score"] / den[raw["tmpl_idx"]]
    cen = np.array([MS.centre_of(tmpls[r["tmpl_idx"]], r["transform"]) for r in raw])
    per = [np.hypot(cen[:, 0] - c[0], cen[:, 1] - c[1]) for c in centres]
    dist = np.min(per, axis=0)
    assert len(raw) > 20 and max(q[d < 3].min() for d in per) < MS.MAX_SCORE < q[dist > 8].min()
    res, idx, boxes, frac = R.detect(orc.volume(), orc.keys, orc.translation, tmpls, raw, 0, max_score=MS.MAX_SCORE, permille=300, den=den)
    assert len(res) == 2
    found = sorted(MS.centre_of(tmpls[r["tmpl_idx"]], r["transform"]) for r in res)
    assert all(np.hypot(f[0] - c[0], f[1] - c[1]) < 3.0 for f, c in zip(found, sorted(centres)))
    # without the rule: every record under the threshold, several per instance
    assert len(R.detect(orc.volume(), orc.keys, orc.translation, tmpls, raw, 0, max_score=MS.MAX_SCORE, permille=1000, den=den)[0]) > 4
