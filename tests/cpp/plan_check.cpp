// plan_check.cpp — plan_launch (parsip_amd/csrc/psgpu_plan.h) as a plain host program, for
// tests/test_launch_plan.py.  Reads planner inputs from stdin, one row of integers per run in the
// order of launch_plan_util.IN_COLS, and prints per row what the run launches (launch_all,
// psgpu_host.cpp: kernel and grid of each launch in order, kernels numbered as
// launch_plan_util.KERNELS), the Params fields the plan carries and the launchFlags bits, in the
// order of launch_plan_util.OUT_COLS.
#define PSGPU_MODEL_NO_HIP
#include "psgpu_plan.h"

#include <cstdio>

enum { PRECHECK, PRECHECK_S, MPU, MPU_S, FRONT, FRONT_S, VERTEX, VERTEX_W, FINISH, FINISH_Q, FINISH_P, SURFACE, SURFACE_W,
       I_PRECHECK, I_MPU, I_VERTEX, I_FINISH };

int main() {
    long v[33];
    for (;;) {
        for (int i = 0; i < 33; ++i)
            if (scanf("%ld", &v[i]) != 1) return i == 0 ? 0 : 1;
        psgpu::PlanInput in{};
        int k = 0;
        in.numCUs = (int)v[k++];
        k += 5;  // dims, mpuBegin: the host's brick_layout made `bricks` of them
        in.mpuCount = (uint32_t)v[k - 1];
        in.bricks = (uint64_t)v[k++];
        in.opt.finishQuad = (int)v[k++];
        in.opt.vertexWide = (int)v[k++];
        in.opt.fusedSurface = (int)v[k++];
        in.opt.front = (int)v[k++];
        in.opt.treeSplit = (int)v[k++];
        in.opt.splitMaxQueued = (uint32_t)v[k++];
        in.opt.gridFit = (int)v[k++];
        in.opt.mpuMarginDiv = (int)v[k++];
        in.opt.vertexBlocksPerCU = (int)v[k++];
        in.opt.finishBlocksPerCU = (int)v[k++];
        in.last.haveQueued = v[k++] != 0;
        in.last.lastQueued = (uint32_t)v[k++];
        in.last.lastSubMax = (uint32_t)v[k++];
        in.last.lastV = (uint32_t)v[k++];
        in.alone = v[k++] != 0;
        in.crowded = v[k++] != 0;
        in.mpuTicks = v[k++] != 0;
        in.splittable = v[k++] != 0;
        in.jit = v[k++] != 0;
        in.hasPrecheckS = v[k++] != 0;
        in.hasSurface = v[k++] != 0;
        in.hasSurfaceW = v[k++] != 0;
        in.hasFront = v[k++] != 0;
        in.hasFrontS = v[k++] != 0;
        in.separate = v[k++] != 0;
        in.shortGrid = v[k++] != 0;
        const psgpu::LaunchPlan pl = psgpu::plan_launch(in);

        long L[4][2] = {{-1, 0}, {-1, 0}, {-1, 0}, {-1, 0}};
        int n = 0;
        const auto launch = [&](int kernel, uint32_t grid) { L[n][0] = kernel, L[n][1] = grid, ++n; };
        const bool J = in.jit;
        if (pl.front) {
            launch(pl.split ? FRONT_S : FRONT, pl.preBlocks + pl.mpuBlocks);
        } else {
            launch(!J ? I_PRECHECK : pl.split ? PRECHECK_S : PRECHECK, pl.preBlocks);
            launch(!J ? I_MPU : pl.split ? MPU_S : MPU, pl.mpuBlocks);
        }
        if (pl.surface) {
            launch(pl.surfaceWide ? SURFACE_W : SURFACE, pl.gridSurface);
        } else {
            launch(!J ? I_VERTEX : pl.vpwVertex == 64 ? VERTEX_W : VERTEX, pl.gridVertex);
            launch(!J ? I_FINISH : pl.vpwFinish == 16 ? FINISH_Q : pl.vpwFinish == 32 ? FINISH_P : FINISH, pl.gridFinish);
        }
        printf("%d", n);
        for (int i = 0; i < 4; ++i) printf(" %ld %ld", L[i][0], L[i][1]);
        printf(" %u %u %u %u %u %u %d %d %d\n", J || pl.surface ? 0u : pl.vpwFinish, pl.preBlocks, pl.mpuBlocks, pl.fqCap,
               pl.scanChunks, pl.scanBlocks, (int)pl.split, (int)pl.surface, (int)pl.front);
    }
}
