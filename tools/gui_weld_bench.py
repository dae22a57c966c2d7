"""Cost of the compat mode's welded mesh (psgpu_gui_weld) on the train scene
(tests/golden/train_corrected.scene) at cell size 0.05, in one process:

* the device weld: hipEvents around psgpu_gui_weld's launches (PSGUI_OPT_TIMING), median of 20
  welds after 5 warm-ups: the weld's phases, k_gui_weld_edges, and the blocking call's wall time;
  the shells and the all-zero filter of that weld the same way;
* the only route a caller has without it: exportMesh() + vertex_edges() +
  meshio.weld_by_edges on the host, wall time, median of 3 (and that both give the same bytes).

    python3 tools/gui_weld_bench.py

With --hot CONFIG [--cellsize CS] a hot-path mesh is welded and filtered the same way
(psgpu_weld / psgpu_weld_filter, 3 floats a colour) so that k_weld_emit and k_filter_emit at
colour width 3 stand beside the compat mode's width 4; times per input vertex are printed for
both, since the vertex counts only come close.

    python3 tools/gui_weld_bench.py --hot C3 --cellsize 0.0227

Output committed as profiles/gui_weld_train.txt (DESIGN.md §6 "Compat weld").
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from parsip_amd import gpu, gui, meshio, scene, synth  # noqa: E402

WARMUP, REPS, HOST_REPS = 5, 20, 3
SCENE = os.path.join(ROOT, "tests", "golden", "train_corrected.scene")


def timed_calls(call, times):
    rows, wall, out = [], [], None
    for k in range(WARMUP + REPS):
        t0 = time.perf_counter()
        out = call()
        t1 = time.perf_counter()
        if k >= WARMUP:
            rows.append(times())
            wall.append((t1 - t0) * 1e3)
    return rows, wall, out


def print_phases(rows, per=None):
    for phase in rows[0]:
        vals = [r[phase] for r in rows]
        med = statistics.median(vals)
        tail = f"   {med * 1e6 / per:7.3f} ns / input vertex" if per else ""
        print(f"  {phase:30s} {med:8.4f}   (min {min(vals):.4f}, max {max(vals):.4f}){tail}")


def gui_main(cellsize):
    root = scene.load_scene(SCENE)[0]
    code, tree = gui.compact_blobtree(root)
    assert code >= 0
    p = gui.ParsipOptimized(0, jit=2)
    p.set_timing(True)
    p.setup(tree, cellsize=cellsize)
    info = p.run()
    V = info.ctVertices
    print(f"train scene: cellsize {cellsize}, lattice {list(info.dims)}, {info.ctLatticeMPUs} MPUs, "
          f"{V} vertices, {info.ctTriangles} triangles, jit status {p.jit_status()}")
    rows, wall, winfo = timed_calls(p.weld_info, p.weld_times)
    print(f"psgpu_gui_weld, median of {REPS} after {WARMUP} warm-ups (hipEvents, ms):")
    print_phases(rows, V)
    print(f"  {'psgpu_gui_weld call, wall':30s} {statistics.median(wall):8.4f}   (launches + wait + the counts' read-back)")
    dev_ms = statistics.median(wall)
    rows, wall, sinfo = timed_calls(p.weld_shells, p.weld_shells_times)
    print(f"psgpu_gui_weld_shells + download, median of {REPS} (hipEvents, ms; wall {statistics.median(wall):.3f}):")
    print_phases(rows)
    rows, wall, _ = timed_calls(p.weld_filter, p.weld_filter_times)
    print(f"psgpu_gui_weld_filter (all-zero) + download, median of {REPS} (hipEvents, ms; wall {statistics.median(wall):.3f}):")
    print_phases(rows, winfo.ctVertices)
    w = p.weld()
    print(f"device weld: {winfo.ctInputVertices} -> {winfo.ctVertices} vertices ({winfo.ctSeamVertices} on MPU faces), "
          f"{winfo.ctTriangles} triangles, {meshio.open_edge_count(w.tris)} open edges, "
          f"{int(sinfo.info['ctShells'])} shells ({int(sinfo.info['ctClosedShells'])} closed)")

    def timed(fn):
        ts, out = [], None
        for _ in range(HOST_REPS):
            t0 = time.perf_counter()
            out = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), out

    def host_route():
        m = p.exportMesh()
        return meshio.weld_by_edges(meshio.TriMesh(m.pos, m.tris.astype(np.int64), m.nrm, m.col), p.vertex_edges())

    t_dl, _ = timed(p.exportMesh)
    t_e, _ = timed(p.vertex_edges)
    t_host, (hw, hmap) = timed(host_route)
    t_wd, _ = timed(p.weld)
    print(f"host route, median of {HOST_REPS} (wall, ms):")
    print(f"  {'exportMesh()':52s} {t_dl:10.2f}")
    print(f"  {'vertex_edges()':52s} {t_e:10.2f}")
    print(f"  {'exportMesh() + vertex_edges() + weld_by_edges':52s} {t_host:10.2f}")
    print(f"  {'weld() (device weld + download of the welded mesh)':52s} {t_wd:10.2f}")
    same = (w.pos.tobytes() == hw.pos.tobytes() and w.nrm.tobytes() == hw.nrm.tobytes() and
            w.col.tobytes() == hw.col.tobytes() and (w.tris == hw.tris).all() and (w.vertex_map == hmap).all())
    print(f"device weld == meshio.weld_by_edges: {bool(same)}")
    print(f"host route / psgpu_gui_weld call: {t_host / dev_ms:.0f}x")
    p.close()


def hot_main(name, cellsize):
    model, cs, _ = synth.make_config(name)
    cs = cellsize or cs
    poly = gpu.Polygonizer(0)
    poly.set_option(gpu.OPT_KERNEL_TIMING, 1)
    poly.set_model(model)
    info = poly.run(cs)
    V = info.ctVertices
    print(f"hot path {name}: cellsize {cs}, {info.ctMPUs} MPUs, {V} vertices, {info.ctTriangles} triangles")
    rows, wall, winfo = timed_calls(poly.weld_info, poly.weld_times)
    print(f"psgpu_weld, median of {REPS} after {WARMUP} warm-ups (hipEvents, ms):")
    print_phases(rows, V)
    poly.weld_shells()
    rows, wall, _ = timed_calls(poly.weld_filter, poly.weld_filter_times)
    print(f"psgpu_weld_filter (all-zero) + download, median of {REPS} (hipEvents, ms):")
    print_phases(rows, winfo.ctVertices)
    poly.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--hot", default=None, help="time the hot path's weld and filter of this config instead")
    ap.add_argument("--cellsize", type=float, default=None)
    args = ap.parse_args()
    if args.hot:
        return hot_main(args.hot, args.cellsize)
    return gui_main(args.cellsize or 0.05)


if __name__ == "__main__":
    main()
