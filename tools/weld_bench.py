"""Cost of a watertight indexed mesh of C3 (128^3 cells, 339,820 vertices, 520,224 triangles),
three ways on one box in one script:

* the device weld: hipEvents around psgpu_weld's launches (PSGPU_OPT_KERNEL_TIMING), median of
  20 welds after 5 warm-ups, the whole weld and each launch, and the blocking call's wall time;
* download() + meshio.weld: the only route before the device weld (position bits: it does not
  close the seams at most cell sizes);
* download() + meshio.weld_lattice: the same definition as the device weld, on the host.

It also prints the welded counts and the open edges each weld leaves.  Output committed as
profiles/weld_c3.txt (DESIGN.md §6 "Weld").

    python3 tools/weld_bench.py [CONFIG]
"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from parsip_amd import gpu, meshio, synth  # noqa: E402

WARMUP, REPS, HOST_REPS = 5, 20, 3


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "C3"
    model, cs, _ = synth.make_config(name)
    lo, hi = model.bbox
    poly = gpu.Polygonizer(0)
    poly.set_option(gpu.OPT_KERNEL_TIMING, 1)
    poly.set_model(model)
    info = poly.run(cs)
    print(f"{name}: cellsize {cs}, {info.ctMPUs} MPUs, {info.ctVertices} vertices, {info.ctTriangles} triangles")
    print("polygonization kernels (ms): " + ", ".join(f"{k} {v:.4f}" for k, v in poly.kernel_times().items()))

    rows, wall = [], []
    for k in range(WARMUP + REPS):
        t0 = time.perf_counter()
        winfo = poly.weld_info()
        t1 = time.perf_counter()
        if k >= WARMUP:
            rows.append(poly.weld_times())
            wall.append((t1 - t0) * 1e3)
    print(f"device weld, median of {REPS} after {WARMUP} warm-ups (hipEvents, ms):")
    for phase in rows[0]:
        vals = [r[phase] for r in rows]
        print(f"  {phase:28s} {statistics.median(vals):8.4f}   (min {min(vals):.4f}, max {max(vals):.4f})")
    print(f"  {'psgpu_weld call, wall':28s} {statistics.median(wall):8.4f}   (launches + wait + the counts' read-back)")
    dev_ms = statistics.median([r["weld total"] for r in rows])

    w = poly.weld()
    print(f"device weld: {winfo.ctInputVertices} -> {winfo.ctVertices} vertices ({winfo.ctSeamVertices} on MPU faces), "
          f"{winfo.ctTriangles} triangles, {meshio.open_edge_count(w.tris)} open edges")

    def timed(fn):
        ts, out = [], None
        for _ in range(HOST_REPS):
            t0 = time.perf_counter()
            out = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), out

    def route_bits():
        return meshio.weld(meshio.from_mesh(poly.download()))

    def route_lattice():
        m = poly.download()
        try:
            return meshio.weld_lattice(m, m.vertex_offsets, cs, lo, hi)
        except ValueError as e:  # a root exactly on a lattice corner: positions alone do not tell its edge
            return e

    t_dl, _ = timed(poly.download)
    t_bits, wb = timed(route_bits)
    t_lat, lat = timed(route_lattice)
    print(f"host routes, median of {HOST_REPS} (wall, ms):")
    print(f"  {'download()':36s} {t_dl:10.2f}")
    print(f"  {'download() + meshio.weld':36s} {t_bits:10.2f}   -> {wb.n_vertices} vertices, "
          f"{meshio.open_edge_count(wb.tris)} open edges")
    if isinstance(lat, ValueError):
        print(f"  {'download() + meshio.weld_lattice':36s} {t_lat:10.2f}   -> ValueError: {lat}")
    else:
        wl, vm = lat
        print(f"  {'download() + meshio.weld_lattice':36s} {t_lat:10.2f}   -> {wl.n_vertices} vertices, "
              f"{meshio.open_edge_count(wl.tris)} open edges")
        same = (w.pos.tobytes() == wl.pos.tobytes() and (w.tris == wl.tris).all() and (w.vertex_map == vm).all())
        print(f"device weld == meshio.weld_lattice: {bool(same)}")
    print(f"download() + meshio.weld / device weld: {t_bits / dev_ms:.0f}x")
    poly.close()


if __name__ == "__main__":
    main()
