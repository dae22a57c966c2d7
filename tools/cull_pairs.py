"""Live (box, primitive) pairs of a config under the sphere form and the box form of the culling
predicate (psgpu_model.h cull_one), through the compiled host predicates
(tests/cpp/cullbound_check.cpp; no GPU needed): over the queued MPUs' boxes (7 cs + 0.001) and the
S1 bricks' corner boxes, per primitive type; the bricks no primitive reaches; and the MPUs the
host model of the S1 field bounds proves empty with the sphere-form and the box-form intervals
(every MPU of the lattice is asked, not only S1's survivors).

Usage: python tools/cull_pairs.py [CONFIG[@CELLS] ...]     e.g.  C3  C3@64  C5
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import cullbound_util as U  # noqa: E402
from parsip_amd import synth  # noqa: E402


def table(name: str) -> str:
    cfg, _, cells = name.partition("@")
    model, cs = U.coarse(cfg, int(cells)) if cells else synth.make_config(cfg)[:2]
    c = U.Check(model, "pairs_" + name.replace("@", "_"), cs=cs)
    n = c.counts()
    mpus, bricks = int(c.dims[0] * c.dims[1] * c.dims[2]), int(((c.dims[0] + 1) // 2) * ((c.dims[1] + 1) // 2) * ((c.dims[2] + 1) // 2))

    def pct(a, b):
        return f"{100.0 * (b - a) / a:+.1f} %" if a else "n/a"

    rows = [f"{name}: cell size {cs:.6g}, lattice {c.dims[0]}x{c.dims[1]}x{c.dims[2]}",
            f"{'live (box, primitive) pairs':44s} {'sphere':>9s} {'box':>9s}  change"]
    for where, label, count in (("mpu_boxes", "MPU boxes", mpus), ("brick_boxes", "S1 brick boxes", bricks)):
        for col in U.COLUMNS:
            a, b = n[f"{where}_sphere"][col], n[f"{where}_box"][col]
            what = f"{label} ({count:,})" if col == "all" else f"  ... {col}"
            rows.append(f"{what:44s} {a:9,d} {b:9,d}  {pct(a, b)}")
    a, b = n["dead_bricks_sphere"], n["dead_bricks_box"]
    rows.append(f"{'bricks with no live primitive':44s} {a:9,d} {b:9,d}  {b - a:+d}")
    a, b = n["proven_empty_sphere"], n["proven_empty_box"]
    rows.append(f"{'MPUs the host model of the bounds proves empty':44s} {a:9,d} {b:9,d}  {b - a:+d}")
    return "\n".join(rows)


if __name__ == "__main__":
    for arg in sys.argv[1:] or ["C3"]:
        print(table(arg))
        print()
