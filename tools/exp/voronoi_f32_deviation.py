"""Measure what float32 does to the Voronoi construction's reals: the numpy restatement (arreau_amd/diffusion/voronoi.py:
voronoi_reference) run in float32 against the same run in float64, over every batch of tests/voronoi_cases.py, on the CPU.  The
largest deviation per quantity, relative to its natural scale (4 pi for solid angles and omega_sum, 1 for weights and cn_eff, V/n
for volumes, (V/n)^(2/3) for areas, the cutoff for lengths), goes into voronoi.F32_DEVIATION (every compared atom) and
voronoi.F32_DEVIATION_CLOSED (the atoms that are not OPEN) by hand; the tests allow
voronoi.BOUND_FACTOR = 16 times it.  Only atoms the float64 run GUARDS are compared, and of them those whose integers the two runs
agree on (printed: how many did not; a disagreement there is a deciding comparison the guards missed, not a rounding of a real).

    python tools/exp/voronoi_f32_deviation.py [BATCH ...]

Two JSON lines per batch (every compared atom; the closed ones) and a last one with the maxima over the batches the tables were
made from (cases.OLD_NAMES), in the form of the constant.  The batches at the caps (cases.NEW_NAMES) are measured the same way but
do not enter the maxima: one that exceeds a table gets the row the last line prints for it, the larger of the table's and its own
number per quantity (voronoi.F32_DEVIATION_AT_CAPS), so no bound of an older batch moves."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from arreau_amd.diffusion import voronoi as vo  # noqa: E402
from tests import voronoi_cases as cases  # noqa: E402

PER_FACE = ("face_solid_angle", "face_weight", "face_area", "face_distance")
PER_ATOM = ("omega_sum", "cn_eff", "volume", "max_radius")


def deviation(bt, r64, r32, closed_only=False):
    """{key: largest |float32 - float64| / scale} over the guarded atoms with equal integers (closed_only: of them those that
    are not OPEN: the far, ill-conditioned vertices of an unclosed cell carry most of an area's or a volume's error), their number,
    the disagreeing ones."""
    scale = vo.scales(bt.lattice, bt.counts, bt.params)
    crystal = np.repeat(np.arange(len(bt.counts)), bt.counts)
    same = np.array([r64.cn[a] == r32.cn[a] and r64.atom_flags[a] == r32.atom_flags[a] and np.array_equal(r64.neighbors[a], r32.neighbors[a])
                     for a in range(len(crystal))], dtype=bool)
    use = r64.guarded & same & (((r64.atom_flags & vo.OPEN) == 0) | (not closed_only))
    out = {k: 0.0 for k in PER_FACE + PER_ATOM}
    for a in np.flatnonzero(use):
        k_ = min(int(r64.cn[a]), bt.params.max_faces)
        for k in PER_FACE:
            d = np.abs(getattr(r32, k)[a, :k_].astype(np.float64) - getattr(r64, k)[a, :k_])
            out[k] = max(out[k], float(d.max(initial=0.0) / scale[k][crystal[a]]))
        for k in PER_ATOM:
            d = abs(float(getattr(r32, k)[a]) - float(getattr(r64, k)[a]))
            out[k] = max(out[k], d / scale[k][crystal[a]])
    return out, int(use.sum()), int((r64.guarded & ~same).sum())


def main():
    top, top_closed, rows = {}, {}, {}
    for name in sys.argv[1:] or cases.NAMES:
        bt, r64 = cases.reference(name)
        r32 = vo.voronoi_reference(bt.frac, bt.lattice, bt.counts, bt.params, dtype=np.float32)
        dev, used, differ = deviation(bt, r64, r32)
        print(json.dumps({"batch": name, "atoms": len(r64.cn), "compared": used, "guarded_but_different_integers": differ, **dev}), flush=True)
        closed, n_closed, _ = deviation(bt, r64, r32, closed_only=True)
        print(json.dumps({"batch": name, "closed_compared": n_closed, **closed}), flush=True)
        if name in cases.NEW_NAMES:
            if any(closed[k] > vo.F32_DEVIATION_CLOSED[k] or dev[k] > vo.F32_DEVIATION[k] for k in dev):
                rows[name] = ({k: max(vo.F32_DEVIATION_CLOSED[k], closed[k]) for k in dev}, {k: max(vo.F32_DEVIATION[k], dev[k]) for k in dev})
            continue
        for k, v in dev.items():
            top[k], top_closed[k] = max(top.get(k, 0.0), v), max(top_closed.get(k, 0.0), closed[k])
    print(json.dumps({"F32_DEVIATION": top, "F32_DEVIATION_CLOSED": top_closed, "F32_DEVIATION_AT_CAPS": rows, "bound_factor": vo.BOUND_FACTOR}), flush=True)


if __name__ == "__main__":
    main()
