"""The run-verdict table (tests/golden/run_verdict.json): finished runs as psgpu_finish sees them
-- the counters k_finish published, the plan the run was launched with, the range's MPU count and
the context's four capacities -- and what the last commit that judged them inline in psgpu_finish
(ed6925b) made of each: fits or not, the next run's LastRun, the grown capacities and the
PsMeshInfo.  The expected rows were recorded from that commit's attempt-loop body and PsMeshInfo
fill, compiled verbatim into a throwaway host program around a stand-in context, so they owe
nothing to judge_run, grown and mesh_info (parsip_amd/csrc/psgpu_plan.h).

cases() builds the inputs; tests/cpp/run_verdict_check.cpp reads them as text."""

IN_COLS = ["mpuCount", "front", "split", "surface", "sieve", "mpb", "mpuBlocks", "vcap", "tcap", "vShardCap", "tShardCap",
           "error", "surfaceErr", "firstOverflow", "reran"]
OUT_COLS = ["fits", "gridShort", "protocol", "haveQueued", "lastQueued", "lastSubMax", "lastV", "usedV", "usedT",
            "usedShardV", "usedShardT", "grownV", "grownT", "grownShardV", "grownShardT", "ctMPUs", "ctPassedPrecheck",
            "ctSurfaceMPUs", "ctVertices", "ctTriangles", "firstOverflowMPU", "ctFieldMPUs", "ctLaneEvals", "launchFlags"]
NO_OVERFLOW = 0x7FFFFFFF
FLAG_SPLIT, FLAG_SURFACE, FLAG_FRONT, FLAG_RERUN, FLAG_SIEVE = 1, 2, 4, 8, 16


def case(shards, **kw):
    """shards: {index: (p, v, t, s, b)}; kw overrides the defaults of a run that fits."""
    d = dict(mpuCount=1000, front=0, split=0, surface=0, sieve=0, mpb=4, mpuBlocks=100, vcap=1 << 20, tcap=1 << 21,
             vShardCap=1 << 15, tShardCap=1 << 16, error=0, surfaceErr=0, firstOverflow=NO_OVERFLOW, reran=0)
    assert set(kw) <= set(d), kw
    d.update(kw)
    return [d[k] for k in IN_COLS], {int(k): tuple(int(x) for x in v) for k, v in shards.items()}


def cases():
    """name -> (inputs, shards), in a fixed order."""
    out = {}
    # a mesh of 640 vertices and 1,280 triangles in 64 equal shards, 4 queued MPUs a shard
    even = {k: (4, 10, 20, 3, 1) for k in range(64)}
    out["fits"] = case(even)
    # each capacity exactly met, and exceeded by one
    out["vcap_met"] = case(even, vcap=640)
    out["vcap_over"] = case(even, vcap=639)
    out["tcap_met"] = case(even, tcap=1280)
    out["tcap_over"] = case(even, tcap=1279)
    lumpy = dict(even)
    lumpy[5] = (4, 5000, 20, 3, 1)
    lumpy[9] = (4, 10, 70000, 3, 1)
    out["vshard_met"] = case(lumpy, vShardCap=5000, tShardCap=70000)
    out["vshard_over"] = case(lumpy, vShardCap=4999, tShardCap=70000)
    out["tshard_met"] = case(lumpy, vShardCap=5000, tShardCap=70000, vcap=5630, tcap=71260)
    out["tshard_over"] = case(lumpy, vShardCap=5000, tShardCap=69999)
    out["all_over"] = case(lumpy, vcap=64, tcap=64, vShardCap=16, tShardCap=32)
    # the plain grid: 256 queued against mpb * mpuBlocks
    one_more = dict(even)
    one_more[63] = (5, 10, 20, 3, 1)
    out["grid_met"] = case(even, mpb=4, mpuBlocks=64)
    out["grid_over"] = case(one_more, mpb=4, mpuBlocks=64)
    out["grid_met_split"] = case(even, mpb=2, mpuBlocks=128, split=1)
    out["grid_over_split"] = case(one_more, mpb=2, mpuBlocks=128, split=1)
    # k_front: sub-queues (shards 0-7) against mpb * (mpuBlocks / 8), mpuBlocks no multiple of 8:
    # 4 * (43 / 8) = 20 a sub-queue, while the plain bound is 4 * 43 = 172
    subs = {k: (12, 10, 20, 3, 1) for k in range(8)}
    subs[3] = (20, 10, 20, 3, 1)
    out["front_met"] = case(subs, front=1, mpb=4, mpuBlocks=43)
    subs[3] = (21, 10, 20, 3, 1)  # one sub-queue over, the sum (105) far under the plain bound
    out["front_over"] = case(subs, front=1, mpb=4, mpuBlocks=43)
    out["front_over_as_plain"] = case(subs, front=0, mpb=4, mpuBlocks=43)
    late = dict(subs)
    late[3] = (20, 10, 20, 3, 1)
    late[8] = (500, 10, 20, 3, 1)  # shard 8 is no sub-queue: k_front counts shards 0-7 only
    out["front_shard8"] = case(late, front=1, mpb=4, mpuBlocks=43)
    out["front_split_over"] = case(subs, front=1, split=1, mpb=2, mpuBlocks=87)  # 2 * 10 = 20 < 21
    out["front_split_fits"] = case(subs, front=1, split=1, mpb=2, mpuBlocks=88)  # 2 * 11 = 22
    # an empty range launches nothing: stale counters, errors included, are neither a short grid nor
    # a protocol error, and its PsMeshInfo is all zero
    stale = {k: (9999, 1 << 21, 1 << 22, 77, 5) for k in range(64)}
    out["empty_stale"] = case(stale, mpuCount=0, mpuBlocks=1, error=1, surfaceErr=2, firstOverflow=17, reran=1,
                              front=1, split=1, surface=1, sieve=1)
    out["empty_clean"] = case({}, mpuCount=0)
    out["nothing_found"] = case({})
    # protocol errors
    out["error"] = case(even, error=1)
    out["surface_err"] = case(even, surfaceErr=2, surface=1)
    out["both_errors"] = case(even, error=1, surfaceErr=2, surface=1, front=1, mpuBlocks=800)
    out["error_and_short"] = case(even, error=1, mpuBlocks=1)
    # firstOverflow
    out["overflow_set"] = case(even, firstOverflow=123456)
    out["overflow_mpu0"] = case(even, firstOverflow=0)
    # every launchFlags bit alone, and all
    out["flag_split"] = case(even, split=1, mpb=2, mpuBlocks=500)
    out["flag_surface"] = case(even, surface=1)
    out["flag_front"] = case(even, front=1, mpuBlocks=800)
    out["flag_rerun"] = case(even, reran=1)
    out["flag_sieve"] = case(even, sieve=1)
    out["flag_all"] = case(even, split=1, surface=1, front=1, reran=1, sieve=1, mpb=2, mpuBlocks=800)
    # sums near 2^32: the growth formulas in 32 bits
    big = {k: (4, 60_000_000, 67_000_000, 3, 1) for k in range(64)}
    out["big"] = case(big, vcap=1 << 30, tcap=0xFFFFFFFF, vShardCap=1 << 26, tShardCap=1 << 26)
    return out


def text(rows):
    """The stdin of run_verdict_check for rows of (inputs, shards)."""
    lines = []
    for inputs, shards in rows:
        flat = [x for k in sorted(shards) for x in (k, *shards[k])]
        lines.append(" ".join(str(int(x)) for x in (*inputs, len(shards), *flat)))
    return "\n".join(lines) + "\n"


def check_coverage(table):
    """table: name -> (inputs, shards, expected row).  The cases the verdict must be pinned at."""
    def row(name):
        i, _, o = table[name]
        return dict(zip(IN_COLS, i)), dict(zip(OUT_COLS, o))

    for stem, cap, used in (("vcap", "vcap", "usedV"), ("tcap", "tcap", "usedT"), ("vshard", "vShardCap", "usedShardV"),
                            ("tshard", "tShardCap", "usedShardT")):
        i, o = row(f"{stem}_met")
        assert i[cap] == o[used] and o["fits"] == 1, (cap, i, o)
        i, o = row(f"{stem}_over")
        assert i[cap] + 1 == o[used] and o["fits"] == 0 and o["gridShort"] == 0, (cap, i, o)
    for met, over in (("grid_met", "grid_over"), ("grid_met_split", "grid_over_split")):
        i, o = row(met)
        assert o["lastQueued"] == i["mpb"] * i["mpuBlocks"] and o["fits"] == 1 and i["front"] == 0
        i, o = row(over)
        assert o["lastQueued"] == i["mpb"] * i["mpuBlocks"] + 1 and (o["fits"], o["gridShort"]) == (0, 1)
    i, o = row("front_met")
    assert i["mpuBlocks"] % 8 and o["lastSubMax"] == i["mpb"] * (i["mpuBlocks"] // 8) and o["fits"] == 1
    i, o = row("front_over")
    assert o["lastSubMax"] == i["mpb"] * (i["mpuBlocks"] // 8) + 1 and (o["fits"], o["gridShort"]) == (0, 1)
    assert o["lastQueued"] < i["mpb"] * i["mpuBlocks"]
    assert row("front_over_as_plain")[1]["fits"] == 1 and row("front_over_as_plain")[1]["lastSubMax"] == 0
    i, o = row("empty_stale")
    # (the capacities are still compared: enqueue zeroes an empty run's counters, so that never bites)
    assert i["mpuCount"] == 0 and i["error"] and i["surfaceErr"] and (o["gridShort"], o["protocol"]) == (0, 0)
    assert row("empty_clean")[1]["fits"] == 1
    assert all(o[k] == 0 for k in ("ctMPUs", "ctVertices", "ctTriangles", "ctLaneEvals", "launchFlags", "haveQueued"))
    assert o["firstOverflowMPU"] == -1 and o["usedV"] > i["vcap"]
    assert row("error")[1]["protocol"] == 1 and row("surface_err")[1]["protocol"] == 2
    assert row("both_errors")[1]["protocol"] == 3 and row("fits")[1]["protocol"] == 0
    assert row("overflow_set")[1]["firstOverflowMPU"] == 123456 and row("overflow_mpu0")[1]["firstOverflowMPU"] == 0
    assert row("fits")[1]["firstOverflowMPU"] == -1
    for name, flag in (("flag_split", FLAG_SPLIT), ("flag_surface", FLAG_SURFACE), ("flag_front", FLAG_FRONT),
                       ("flag_rerun", FLAG_RERUN), ("flag_sieve", FLAG_SIEVE), ("flag_all", 31), ("fits", 0)):
        assert row(name)[1]["launchFlags"] == flag, name
