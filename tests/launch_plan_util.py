"""The launch-plan table (tests/golden/launch_plan.npz): its columns, and the conditions that keep
it from missing a branch of plan_launch (parsip_amd/csrc/psgpu_plan.h).

Every row is one run's planner input and what the last commit without the planner (e7ba9eb: five
predicates over the context, grid arithmetic in make_params and launch_all) did with it: which
kernel each launch took, in order, and its grid; the Params fields the plan now carries; the three
launchFlags bits.  It was recorded from that commit's psgpu_host.cpp itself, compiled into a
throwaway host program with a hipModuleLaunchKernel that writes down (function, grid) and a
hand-filled context, so the expected columns owe nothing to the planner."""
import numpy as np

IN_COLS = ["numCUs", "dims0", "dims1", "dims2", "mpuBegin", "mpuCount", "bricks", "finishQuad", "vertexWide",
           "fusedSurface", "front", "treeSplit", "splitMaxQueued", "gridFit", "mpuMarginDiv", "vertexBlocksPerCU",
           "finishBlocksPerCU", "haveQueued", "lastQueued", "lastSubMax", "lastV", "alone", "crowded", "mpuTicks",
           "splittable", "jit", "hasPrecheckS", "hasSurface", "hasSurfaceW", "hasFront", "hasFrontS", "separate",
           "shortGrid"]
# launches: kernel (an index into KERNELS, -1: none) and grid of each of up to four, in order;
# interpFinishVpw: the layout handed to the interpreter's k_finish (0: generated kernels)
OUT_COLS = ["launches", "k0", "g0", "k1", "g1", "k2", "g2", "k3", "g3", "interpFinishVpw", "preBlocks", "mpuBlocks",
            "fqCap", "scanChunks", "scanBlocks", "flagSplit", "flagSurface", "flagFront"]
KERNELS = ["precheck", "precheckS", "mpu", "mpuS", "front", "frontS", "vertex", "vertexW", "finish", "finishQ",
           "finishP", "surface", "surfaceW", "interp_precheck", "interp_mpu", "interp_vertex", "interp_finish"]


def check_coverage(inputs: np.ndarray, expected: np.ndarray) -> None:
    i = {k: inputs[:, n].astype(np.int64) for n, k in enumerate(IN_COLS)}
    o = {k: expected[:, n].astype(np.int64) for n, k in enumerate(OUT_COLS)}

    def need(mask, what):
        assert np.any(mask), f"no row with {what}"

    def around(col, value, where, what):
        for d in (-1, 0, 1):
            need(where & (col == value + d), f"{what} at {value} {d:+d}")

    def launched(*names):  # per row: the grid of the launch that took one of `names`, or -1
        grid = np.full(len(inputs), -1, np.int64)
        for s in range(4):
            hit = np.isin(o[f"k{s}"], [KERNELS.index(n) for n in names])
            grid[hit] = o[f"g{s}"][hit]
        return grid

    for n, name in enumerate(KERNELS):
        need(np.any([o[f"k{s}"] == n for s in range(4)], axis=0), f"a launch of {name}")

    std = (i["numCUs"] == 256) & (i["vertexBlocksPerCU"] == 16) & (i["finishBlocksPerCU"] == 8)
    jit = i["jit"] == 1
    for waves in (16, 32):
        around(i["lastV"], waves * 256 * 8 * 4, std & (i["finishQuad"] == 2), f"k_finish: lastV, {waves} per wave")
    around(i["lastV"], 16 * 256 * 16 * 4, std & jit & (i["vertexWide"] == 2) & (i["alone"] == 0), "k_vertex: lastV")
    around(i["lastV"], 16 * 8 * 24 * 256, std & jit & (i["alone"] == 1) & (i["fusedSurface"] == 2) & (i["hasSurface"] == 1)
           & (i["separate"] == 0) & (i["crowded"] == 0), "loneMaxV: lastV")
    around(i["lastQueued"] - i["splitMaxQueued"], 0, std & jit & (i["treeSplit"] == 2) & (i["haveQueued"] == 1)
           & (i["hasPrecheckS"] == 1) & (i["splittable"] == 1), "lastQueued - splitMaxQueued")
    for split in (0, 1):
        around(o["preBlocks"], 8 * 256, std & jit & (i["front"] == 2) & (o["flagSplit"] == split) & (i["hasFront"] == 1)
               & (i["hasFrontS"] == 1) & (i["separate"] + i["crowded"] + i["mpuTicks"] == 0), f"preBlocks, split {split}")

    # the fitted grids before clamping, against the persistent grids and scanBlocks
    fit = (i["gridFit"] == 1) & (i["lastV"] > 0)
    vv = i["lastV"] + i["lastV"] // 8 + 256
    for names, per, cap, scan in ((("vertex", "interp_vertex"), 64, "vertexBlocksPerCU", True),
                                  (("vertexW",), 256, "vertexBlocksPerCU", True), (("finishQ",), 64, "finishBlocksPerCU", False),
                                  (("finishP",), 128, "finishBlocksPerCU", False), (("finish",), 256, "finishBlocksPerCU", False),
                                  (("surface",), 64, "vertexBlocksPerCU", True), (("surfaceW",), 256, "finishBlocksPerCU", True)):
        took = fit & (launched(*names) >= 0)
        around((vv + per - 1) // per - i["numCUs"] * i[cap], 0, took & std, f"{names[0]}: fitted grid - its cap")
        if scan:
            around((vv + per - 1) // per - o["scanBlocks"], 0, took, f"{names[0]}: fitted grid - scanBlocks")
    need(o["scanChunks"] > 1, "scanChunks > 1")
    need(o["scanBlocks"] > i["numCUs"] * i["vertexBlocksPerCU"], "scanBlocks over the persistent grid")

    mpb = np.where(o["flagSplit"] == 1, 2, 4)
    plain = (o["flagFront"] == 0) & (i["haveQueued"] == 1) & (i["shortGrid"] == 0)
    for div, plus in ((4, 256), (8, 64)):
        want = (i["lastQueued"] + i["lastQueued"] // div + plus + mpb - 1) // mpb
        around(want - (i["mpuCount"] + mpb - 1) // mpb, 0, plain & (i["mpuMarginDiv"] == div), f"k_mpu blocks - maxBlocks, 1/{div}")
    sub = np.where(i["lastSubMax"] > 0, i["lastSubMax"], (i["lastQueued"] + 7) // 8) + i["lastQueued"] // 32 + 32
    fronted = (o["flagFront"] == 1) & (i["haveQueued"] == 1)
    for short in (0, 1):
        around(sub - o["fqCap"], 0, fronted & (i["shortGrid"] == short), f"k_front rows - fqCap, shortGrid {short}")
    need(fronted & (i["lastSubMax"] == 0), "lastSubMax 0 with k_front")
    need((o["flagFront"] == 1) & (i["haveQueued"] == 0), "k_front without a last run")

    for name, values in (("finishQuad", range(4)), ("vertexWide", range(3)), ("fusedSurface", range(4)), ("front", range(3)),
                         ("treeSplit", range(3)), ("gridFit", (0, 1)), ("mpuMarginDiv", (4, 8)), ("alone", (0, 1)),
                         ("crowded", (0, 1)), ("separate", (0, 1)), ("mpuTicks", (0, 1)), ("shortGrid", (0, 1)),
                         ("haveQueued", (0, 1)), ("numCUs", (256, 64))):
        for v in values:
            for j in (0, 1):  # on the generated kernels and on the interpreter
                need((i[name] == v) & (i["jit"] == j), f"{name} {v}, jit {j}")
    need(jit & (i["hasPrecheckS"] == 0) & (i["treeSplit"] == 1), "a module without the split kernels, split asked for")
    need(jit & (i["hasSurface"] == 1) & (i["hasSurfaceW"] == 0) & (i["fusedSurface"] == 3), "a module without surfaceW, asked for")
    need(jit & (i["hasFront"] == 0) & (i["hasFrontS"] == 0) & (i["front"] == 1), "a module without the front kernels, asked for")
    need(i["mpuBegin"] != 0, "mpuBegin != 0")
    for flag in ("flagSplit", "flagSurface", "flagFront"):
        for v in (0, 1):
            need(o[flag] == v, f"{flag} {v}")
