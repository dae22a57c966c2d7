// run_verdict_check.cpp — judge_run, grown and mesh_info (parsip_amd/csrc/psgpu_plan.h) as a
// plain host program, for tests/test_launch_plan.py.  Reads one finished run per row from stdin:
// the integers of run_verdict_util.IN_COLS, then a count n and n shards as (index, p, v, t, s, b);
// the other shards' counters are zero.  Prints per row the verdict, the grown capacities and the
// PsMeshInfo in the order of run_verdict_util.OUT_COLS.
#define PSGPU_MODEL_NO_HIP
#include "psgpu_plan.h"

#include <cstdio>
#include <memory>

int main() {
    std::unique_ptr<psgpu::DevCounters> h(new psgpu::DevCounters);
    long v[15];
    for (;;) {
        for (int i = 0; i < 15; ++i)
            if (scanf("%ld", &v[i]) != 1) return i == 0 ? 0 : 1;
        memset(h.get(), 0, sizeof(psgpu::DevCounters));
        psgpu::LaunchPlan run{};
        int k = 0;
        const uint32_t mpuCount = (uint32_t)v[k++];
        run.front = v[k++] != 0;
        run.split = v[k++] != 0;
        run.surface = v[k++] != 0;
        run.sieve = (uint32_t)v[k++];
        run.mpb = (uint32_t)v[k++];
        run.mpuBlocks = (uint32_t)v[k++];
        psgpu::Caps caps;
        caps.v = (uint32_t)v[k++];
        caps.t = (uint32_t)v[k++];
        caps.shardV = (uint32_t)v[k++];
        caps.shardT = (uint32_t)v[k++];
        h->error = (uint32_t)v[k++];
        h->surfaceErr = (uint32_t)v[k++];
        h->firstOverflow = (int32_t)v[k++];
        const bool reran = v[k++] != 0;
        long n = 0;
        if (scanf("%ld", &n) != 1 || n < 0 || n > psgpu::kShards) return 1;
        for (long j = 0; j < n; ++j) {
            long s[6];
            for (long& x : s)
                if (scanf("%ld", &x) != 1) return 1;
            if (s[0] < 0 || s[0] >= psgpu::kShards) return 1;
            psgpu::ShardCtr& c = h->shard[s[0]];
            c.p = (uint32_t)s[1], c.v = (uint32_t)s[2], c.t = (uint32_t)s[3], c.s = (uint32_t)s[4], c.b = (uint32_t)s[5];
        }
        const psgpu::RunVerdict r = psgpu::judge_run(*h, run, mpuCount, caps);
        const psgpu::Caps g = psgpu::grown(caps, r);
        const PsMeshInfo I = psgpu::mesh_info(*h, run, mpuCount, reran);
        printf("%d %d %u %d %u %u %u %u %u %u %u %u %u %u %u", (int)r.fits, (int)r.gridShort, r.protocol, (int)r.last.haveQueued,
               r.last.lastQueued, r.last.lastSubMax, r.last.lastV, r.used.v, r.used.t, r.used.shardV, r.used.shardT, g.v, g.t,
               g.shardV, g.shardT);
        printf(" %u %u %u %u %u %d %u %llu %u\n", I.ctMPUs, I.ctPassedPrecheck, I.ctSurfaceMPUs, I.ctVertices, I.ctTriangles,
               I.firstOverflowMPU, I.ctFieldMPUs, (unsigned long long)I.ctLaneEvals, I.launchFlags);
    }
}
