"""CPU model of the S2 octant walk (DESIGN.md §4 "S2 octants"): for a config, which octants of
each queued MPU S1's field bounds decide, and what S2 then walks.  No GPU needed: the S1 verdicts
come from the CPU oracle, the per-octant verdicts from the host program
tests/cpp/s2_octants_check.cpp (the device's expressions compiled as plain C++).

Usage: python tools/s2_octants.py [--configs C2,C3,C5] [--json FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, d)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C3,C5")
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    a = ap.parse_args()
    import psoracle
    import s2_octants_util as S
    from parsip_amd import synth

    psoracle.build()
    rows = {}
    for name in a.configs.split(","):
        model, cs = synth.make_config(name)[:2]  # (an animated config: its frame 0)
        om = psoracle.polygonize(model, cs, threads=os.cpu_count() or 1, keep=False)
        v = S.Verdicts(model, cs, om.stats[:, 0], "tool_" + name)
        r = rows[name] = v.counts()
        passed = int((om.stats[:, 0] != 0).sum())
        n = max(r["queued"], 1)
        one, two = int((v.passes[v.queued] == 1).sum()), int((v.passes[v.queued] == 2).sum())
        print(f"{name}: {passed} passed S1, {passed - r['queued']} proven empty, {r['queued']} queued")
        print(f"  undecided octants per queued MPU, histogram 0..8: {' '.join(map(str, r['undecided_histogram']))}")
        print(f"  mean undecided octants (of 8): {r['mean_undecided']:.2f}")
        print(f"  queued MPUs with <= 4 undecided: {100.0 * r['queued_le4_undecided'] / n:.1f} %")
        print(f"  S2 lattice points: {r['points_all']}, in octants S1 decided: {r['points_decided']} "
              f"({100.0 * r['points_decided'] / max(r['points_all'], 1):.1f} %)")
        print(f"  4-octant walks: {r['passes']} ({one} MPUs take one, {two} take two, "
              f"{r['queued'] - one - two} none) against {r['passes_all_octants']}: "
              f"{100.0 * (1.0 - r['passes'] / max(r['passes_all_octants'], 1)):.1f} % fewer points walked")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
