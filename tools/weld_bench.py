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

With --parts N the same input runs as a Group of N parts on device 0 (the default, planned
split) and psgpu_group_weld is timed the same way, each of its phases, beside the
single-context weld of the same input in the same process and the only route a group had
before: Group.download() + meshio.weld.  Output of --parts 1, 2 and 8 committed as
profiles/group_weld_c3.txt (DESIGN.md §6 "Weld of a group").

    python3 tools/weld_bench.py [CONFIG] --parts N

With --shells the shells of the weld are timed (psgpu_weld_shells: hipEvents through
psgpu_weld_shells_times, the whole call and each step, median of 20 after 5 warm-ups), beside
the weld re-measured in the same process and the host route download of the weld +
meshio.shells.  Output committed as profiles/shells_c3.txt (DESIGN.md §6 "Shells").

    python3 tools/weld_bench.py [CONFIG] --shells

With --filter the filter of the weld by its shells is timed (psgpu_weld_filter: hipEvents
through psgpu_weld_filter_times, the whole call and each launch, median of 20 after 5 warm-ups)
with minTriangles midway between the two largest shells (the body stays, the bits around it go),
beside the weld re-measured in the same process and the host route: downloads of the weld and
the shells + meshio.filter_shells.  Output committed as profiles/filter_c3.txt (DESIGN.md §6
"Filter").

    python3 tools/weld_bench.py [CONFIG] --filter
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from parsip_amd import gpu, meshio, soa, synth  # noqa: E402

WARMUP, REPS, HOST_REPS = 5, 20, 3


def timed_welds(weld_info, weld_times):
    """Per-phase hipEvent times and the blocking call's wall time (ms) of REPS welds after WARMUP."""
    rows, wall, winfo = [], [], None
    for k in range(WARMUP + REPS):
        t0 = time.perf_counter()
        winfo = weld_info()
        t1 = time.perf_counter()
        if k >= WARMUP:
            rows.append(weld_times())
            wall.append((t1 - t0) * 1e3)
    return rows, wall, winfo


def print_phases(rows):
    for phase in rows[0]:
        vals = [r[phase] for r in rows]
        print(f"  {phase:28s} {statistics.median(vals):8.4f}   (min {min(vals):.4f}, max {max(vals):.4f})")


def group_main(name, parts):
    model, cs, _ = synth.make_config(name)
    poly = gpu.Polygonizer(0)
    poly.set_option(gpu.OPT_KERNEL_TIMING, 1)
    poly.set_model(model)
    info = poly.run(cs)
    print(f"{name}: cellsize {cs}, {info.ctMPUs} MPUs, {info.ctVertices} vertices, {info.ctTriangles} triangles")
    rows, wall, _ = timed_welds(poly.weld_info, poly.weld_times)
    print(f"single-context weld, median of {REPS} after {WARMUP} warm-ups (hipEvents, ms):")
    print_phases(rows)
    print(f"  {'psgpu_weld call, wall':28s} {statistics.median(wall):8.4f}")
    one_ms = statistics.median([r["weld total"] for r in rows])
    one = poly.weld()

    g = gpu.Group([0] * parts)
    g.set_option(gpu.OPT_KERNEL_TIMING, 1)
    g.set_model(model)
    total, pinfo = g.run(cs)
    print(f"group of {parts} part(s) on device 0, MPU bounds {g.split().tolist()}, "
          f"vertices per part {[p.info.ctVertices for p in pinfo]}")
    rows, wall, winfo = timed_welds(g.weld_info, g.weld_times)
    print(f"group weld, median of {REPS} after {WARMUP} warm-ups (hipEvents on the gathering stream, ms):")
    print_phases(rows)
    print(f"  {'psgpu_group_weld call, wall':28s} {statistics.median(wall):8.4f}   (launches + wait + the counts' read-back)")
    med = {ph: statistics.median([r[ph] for r in rows]) for ph in rows[0]}
    grp_ms = med["group weld total"]
    top = max((ph for ph in med if ph != "group weld total"), key=lambda ph: med[ph])
    print(f"  largest phase: {top} ({med[top]:.4f} ms, {100 * med[top] / grp_ms:.0f} % of the total)")
    w = g.weld()
    same = all(np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()
               for a, b in ((w.pos, one.pos), (w.nrm, one.nrm), (w.col, one.col), (w.tris, one.tris),
                            (w.vertex_map, one.vertex_map)))
    print(f"group weld: {winfo.ctInputVertices} -> {winfo.ctVertices} vertices ({winfo.ctSeamVertices} on MPU faces), "
          f"{winfo.ctTriangles} triangles, {meshio.open_edge_count(w.tris)} open edges; "
          f"bytes equal the single-context weld: {bool(same)}")

    ts, wb = [], None
    for _ in range(HOST_REPS):
        t0 = time.perf_counter()
        wb = meshio.weld(meshio.from_mesh(g.download()))
        ts.append((time.perf_counter() - t0) * 1e3)
    host_ms = statistics.median(ts)
    print(f"host route, median of {HOST_REPS} (wall, ms):")
    print(f"  {'Group.download() + meshio.weld':36s} {host_ms:10.2f}   -> {wb.n_vertices} vertices, "
          f"{meshio.open_edge_count(wb.tris)} open edges")
    print(f"group weld / single-context weld: {grp_ms / one_ms:.2f}x; "
          f"Group.download() + meshio.weld / group weld: {host_ms / grp_ms:.0f}x")
    g.close()
    poly.close()


def shells_main(name):
    model, cs, _ = synth.make_config(name)
    poly = gpu.Polygonizer(0)
    poly.set_option(gpu.OPT_KERNEL_TIMING, 1)
    poly.set_model(model)
    info = poly.run(cs)
    print(f"{name}: cellsize {cs}, {info.ctMPUs} MPUs, {info.ctVertices} vertices, {info.ctTriangles} triangles")
    rows, wall, winfo = timed_welds(poly.weld_info, poly.weld_times)
    print(f"device weld, median of {REPS} after {WARMUP} warm-ups (hipEvents, ms):")
    print_phases(rows)
    print(f"  {'psgpu_weld call, wall':28s} {statistics.median(wall):8.4f}")
    weld_ms = statistics.median([r["weld total"] for r in rows])

    L = gpu.load()
    sinfo = gpu.PsShellsInfo()

    def shells_info():
        rc = L.psgpu_weld_shells(poly._ctx, sinfo)
        assert rc == soa.RET_SUCCESS, rc
        return sinfo

    rows, wall, _ = timed_welds(shells_info, poly.weld_shells_times)
    print(f"device shells, median of {REPS} after {WARMUP} warm-ups (hipEvents, ms; the total and the "
          "k_shells_ids row include the host's read of the shell count between the two halves):")
    print_phases(rows)
    print(f"  {'psgpu_weld_shells call, wall':28s} {statistics.median(wall):8.4f}")
    med = {ph: statistics.median([r[ph] for r in rows]) for ph in rows[0]}
    dev_ms = med["shells total"]
    top = max((ph for ph in med if ph != "shells total"), key=lambda ph: med[ph])
    print(f"  largest phase: {top} ({med[top]:.4f} ms, {100 * med[top] / dev_ms:.0f} % of the total)")
    acc = med["k_shells_vertices"] + med["k_shells_edge_class"] + med["k_shells_triangles"]
    print(f"  the three accumulate kernels: {acc:.4f} ms ({100 * acc / dev_ms:.0f} % of the total)")
    sh = poly.weld_shells()
    i = sh.info
    print(f"shells: {i['ctShells']} ({i['ctClosedShells']} closed), V {i['ctVertices']} T {i['ctTriangles']} "
          f"E {i['ctEdges']}, open {i['ctOpenEdges']}, non-manifold {i['ctNonManifoldEdges']}, "
          f"flipped {i['ctFlippedEdges']}, euler {i['euler']}, area {float(i['area']):.12g}, "
          f"volume {float(i['volume']):.12g}")
    for s in sh.shells[:8]:
        print(f"  shell first vertex {s['firstVertex']}: V {s['ctVertices']} T {s['ctTriangles']} E {s['ctEdges']} "
              f"open {s['ctOpenEdges']} euler {s['euler']} area {float(s['area']):.9g} volume {float(s['volume']):.9g}")

    ts, ref = [], None
    for _ in range(HOST_REPS):
        t0 = time.perf_counter()
        w = poly.weld()
        t1 = time.perf_counter()
        ref = meshio.shells(w.pos, w.tris)
        ts.append(((t1 - t0) * 1e3, (time.perf_counter() - t0) * 1e3))
    dl_ms, host_ms = (statistics.median(c) for c in zip(*ts))
    print(f"host route, median of {HOST_REPS} (wall, ms):")
    print(f"  {'weld() (weld + download)':36s} {dl_ms:10.2f}")
    print(f"  {'weld() + meshio.shells':36s} {host_ms:10.2f}")
    print(f"device shells == meshio.shells: {sh.tobytes() == ref.tobytes()}")
    print(f"shells / weld on the device: {dev_ms / weld_ms:.2f}x; host route / device shells: {host_ms / dev_ms:.0f}x")
    poly.close()


def filter_main(name):
    model, cs, _ = synth.make_config(name)
    poly = gpu.Polygonizer(0)
    poly.set_option(gpu.OPT_KERNEL_TIMING, 1)
    poly.set_model(model)
    info = poly.run(cs)
    print(f"{name}: cellsize {cs}, {info.ctMPUs} MPUs, {info.ctVertices} vertices, {info.ctTriangles} triangles")
    rows, wall, winfo = timed_welds(poly.weld_info, poly.weld_times)
    print(f"device weld, median of {REPS} after {WARMUP} warm-ups (hipEvents, ms):")
    print_phases(rows)
    print(f"  {'psgpu_weld call, wall':28s} {statistics.median(wall):8.4f}")
    wmed = {ph: statistics.median([r[ph] for r in rows]) for ph in rows[0]}
    weld_ms, moved_ms = wmed["weld total"], wmed["k_weld_emit"] + wmed["k_weld_map"]

    sh = poly.weld_shells()
    by_size = np.sort(sh.shells["ctTriangles"])[::-1]
    cut = int((int(by_size[0]) + int(by_size[1] if len(by_size) > 1 else 0)) // 2)
    criteria = meshio.shell_filter(minTriangles=cut)
    print(f"shells: {len(sh.shells)}, triangles per shell {by_size[:10].tolist()}; filter: minTriangles {cut}")
    L = gpu.load()
    finfo = gpu.PsFilterInfo()

    def filter_info():
        rc = L.psgpu_weld_filter(poly._ctx, criteria.ctypes.data, None, 0, finfo)
        assert rc == soa.RET_SUCCESS, rc
        return finfo

    rows, wall, _ = timed_welds(filter_info, poly.weld_filter_times)
    print(f"device filter, median of {REPS} after {WARMUP} warm-ups (hipEvents, ms):")
    print_phases(rows)
    print(f"  {'psgpu_weld_filter call, wall':28s} {statistics.median(wall):8.4f}   (launches + wait + the totals' read-back)")
    med = {ph: statistics.median([r[ph] for r in rows]) for ph in rows[0]}
    dev_ms = med["filter total"]
    top = max((ph for ph in med if ph != "filter total"), key=lambda ph: med[ph])
    print(f"  largest launch: {top} ({med[top]:.4f} ms, {100 * med[top] / dev_ms:.0f} % of the total)")
    compact = med["k_filter_emit"] + med["k_filter_tris"]
    print(f"  k_filter_emit + k_filter_tris: {compact:.4f} ms = {compact / moved_ms:.2f}x k_weld_emit + k_weld_map "
          f"({moved_ms:.4f} ms); filter total / (k_weld_emit + k_weld_map): {dev_ms / moved_ms:.2f}x")
    print(f"filter: {finfo.ctInputShells} -> {finfo.ctShells} shells, {finfo.ctInputVertices} -> {finfo.ctVertices} "
          f"vertices, {finfo.ctInputTriangles} -> {finfo.ctTriangles} triangles")
    f = poly.weld_filter(criteria)

    ts, ref = [], None
    for _ in range(HOST_REPS):
        t0 = time.perf_counter()
        w = poly.weld()
        hs = poly.weld_shells()
        t1 = time.perf_counter()
        ref = meshio.filter_shells(w.pos, w.nrm, w.col, w.tris, hs, criteria)
        ts.append(((t1 - t0) * 1e3, (time.perf_counter() - t0) * 1e3))
    dl_ms, host_ms = (statistics.median(c) for c in zip(*ts))
    print(f"host route, median of {HOST_REPS} (wall, ms; the filtered mesh is not uploaded again):")
    print(f"  {'weld() + weld_shells() (calls + downloads)':44s} {dl_ms:10.2f}")
    print(f"  {'... + meshio.filter_shells':44s} {host_ms:10.2f}")
    print(f"device filter == meshio.filter_shells: {f.tobytes() == ref.tobytes()}")
    print(f"filter / weld on the device: {dev_ms / weld_ms:.2f}x; host route / device filter: {host_ms / dev_ms:.0f}x")
    poly.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("config", nargs="?", default="C3")
    ap.add_argument("--parts", type=int, default=0, help="run as a Group of N parts on device 0 and time psgpu_group_weld")
    ap.add_argument("--shells", action="store_true", help="time psgpu_weld_shells on the weld")
    ap.add_argument("--filter", action="store_true", help="time psgpu_weld_filter on the weld and its shells")
    args = ap.parse_args()
    if args.filter:
        return filter_main(args.config)
    if args.shells:
        return shells_main(args.config)
    if args.parts > 0:
        return group_main(args.config, args.parts)
    name = args.config
    model, cs, _ = synth.make_config(name)
    lo, hi = model.bbox
    poly = gpu.Polygonizer(0)
    poly.set_option(gpu.OPT_KERNEL_TIMING, 1)
    poly.set_model(model)
    info = poly.run(cs)
    print(f"{name}: cellsize {cs}, {info.ctMPUs} MPUs, {info.ctVertices} vertices, {info.ctTriangles} triangles")
    print("polygonization kernels (ms): " + ", ".join(f"{k} {v:.4f}" for k, v in poly.kernel_times().items()))

    rows, wall, winfo = timed_welds(poly.weld_info, poly.weld_times)
    print(f"device weld, median of {REPS} after {WARMUP} warm-ups (hipEvents, ms):")
    print_phases(rows)
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
