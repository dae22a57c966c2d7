// psgpu_filter.hip — the welded mesh filtered by shell: the shells that pass the criteria
// stay, the mesh is compacted in order (psgpu_weld_filter / psgpu_group_weld_filter,
// include/parsip_gpu.h).
//
// The input is a WeldState's welded arrays and the shells result beside them (psgpu_shells.hip),
// a context's or a group's alike.
//
//   k_filter_select  one lane per shell: keep[s] from its PsShell, the criteria and the mask;
//                    kept shells per block
//   k_filter_flags   one lane per welded vertex and per triangle: kept iff its shell is; per
//                    block, kept vertices | kept triangles << 32
//   k_weld_scan      (psgpu_weld.hip) twice: the shells' block counts, the mesh's
//   k_filter_emit    one lane per welded vertex: vertexMap (block_rank + block base), the kept
//                    pos / nrm / col compacted through LDS (compact3); k_filter_emit<4>, the
//                    compat context's rgba colours: one 16-byte load and store a kept vertex
//   k_filter_shells  one lane per shell: shellMap, the kept PsShell records with firstVertex
//                    through vertexMap; the totals into the control words
//   k_filter_tris    one lane per triangle: the kept ones compacted in order as vertexMap[tris]
//                    (stage_in, the map, stage_out)
//
// The counting and compacting stages (block_rank, stage_in / stage_out, compact3) are psgpu_mesh_stages.h's, shared
// with the weld and the shells.
// The phases are ordered by kernel boundaries alone: no block waits for another inside a
// launch, and no kernel has a loop beyond its block's own elements.  Whether an element is
// kept is recomputed from keep[] where it is needed (4 + 1 bytes read) instead of stored.  The
// host reads once, at the end: four control words.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "psgpu_filter_check.h"
#include "psgpu_internal.h"
#include "psgpu_mesh_stages.h"

namespace psgpu {

namespace {

constexpr uint32_t kDropped = 0xffffffffu;  // vertexMap / shellMap of what the filter drops

enum : int { cErr, cShells, cVertices, cTriangles, kCtlWords };  // FilterState::ctl

struct FilterParams {
    const float *pos, *nrm, *col;  // the welded mesh
    const uint32_t* tris;
    const PsShell* shells;  // the shells result
    const uint32_t* vertexShell;
    const uint32_t* triShell;
    uint32_t V, T, S;
    PsShellFilter crit;
    const uint8_t* mask;  // S bytes, or null
    uint8_t* keep;        // S
    uint64_t* shellCnt;   // shellBlocks + 1: kept shells per block of kMeshBlock shells, then scanned
    uint64_t* blockCnt;   // blocks + 1: kept vertices | kept triangles << 32 per block, then scanned
    uint32_t shellBlocks, blocks;
    uint32_t* ctl;
    float *fpos, *fnrm, *fcol;  // the filtered mesh
    uint32_t* ftris;
    uint32_t* vertexMap;
    uint32_t* shellMap;
    PsShell* fshells;
};

__device__ __forceinline__ bool shell_kept(const FilterParams& q, uint32_t s) { return s < q.S && q.keep[s] != 0; }

__global__ void __launch_bounds__(kMeshBlock) k_filter_select(FilterParams q) {
    __shared__ uint32_t sWave[kMeshWaves];
    const uint32_t s = blockIdx.x * kMeshBlock + threadIdx.x;
    bool keep = false;
    if (s < q.S) {
        const PsShell& h = q.shells[s];
        const bool closed = h.ctTriangles > 0u && !h.ctOpenEdges && !h.ctFlippedEdges && !h.ctNonManifoldEdges;
        keep = (q.mask == nullptr || q.mask[s] != 0) && h.ctVertices >= q.crit.minVertices &&
               h.ctTriangles >= q.crit.minTriangles && h.area >= q.crit.minArea &&
               fabs(h.volume) >= q.crit.minAbsVolume;
        if ((q.crit.flags & PSGPU_FILTER_CLOSED_ONLY) && !closed) keep = false;
        if ((q.crit.flags & PSGPU_FILTER_DROP_CAVITIES) && closed && h.volume < 0.0) keep = false;
        q.keep[s] = keep ? 1 : 0;
    }
    uint32_t n;
    (void)block_rank(keep, sWave, &n);
    if (threadIdx.x == 0) q.shellCnt[blockIdx.x] = n;
    if (s == 0u) q.ctl[cErr] = 0u;
}

__global__ void __launch_bounds__(kMeshBlock) k_filter_flags(FilterParams q) {
    __shared__ uint32_t sWave[kMeshWaves];
    const uint32_t i = blockIdx.x * kMeshBlock + threadIdx.x;
    const bool v = i < q.V && shell_kept(q, q.vertexShell[i]);
    const bool t = i < q.T && shell_kept(q, q.triShell[i]);
    uint32_t nv, nt;
    (void)block_rank(v, sWave, &nv);
    __syncthreads();  // sWave is read until every wave has its nv
    (void)block_rank(t, sWave, &nt);
    if (threadIdx.x == 0) q.blockCnt[blockIdx.x] = (uint64_t)nv | (uint64_t)nt << 32;
}

template <int W>  // floats a colour (WeldState::colW)
__global__ void __launch_bounds__(kMeshBlock) k_filter_emit(FilterParams q) {
    __shared__ __attribute__((aligned(16))) uint32_t sIn[3 * kMeshBlock];
    __shared__ uint32_t sOut[3 * kMeshBlock];
    __shared__ uint32_t sWave[kMeshWaves];
    const uint32_t v0 = blockIdx.x * kMeshBlock;
    const uint32_t v = v0 + threadIdx.x;
    const uint32_t n = min(kMeshBlock, q.V - v0);
    const bool kept = v < q.V && shell_kept(q, q.vertexShell[v]);
    uint32_t nKept;
    const uint32_t at = block_rank(kept, sWave, &nKept);
    const uint32_t base = (uint32_t)q.blockCnt[blockIdx.x];
    if (v < q.V) q.vertexMap[v] = kept ? base + at : kDropped;
    if (nKept == 0u) return;  // block-uniform
    compact3(q.pos, q.fpos, v0, n, kept, at, nKept, base, sIn, sOut);
    compact3(q.nrm, q.fnrm, v0, n, kept, at, nKept, base, sIn, sOut);
    if constexpr (W == 3) {
        compact3(q.col, q.fcol, v0, n, kept, at, nKept, base, sIn, sOut);
    } else {
        static_assert(W == 4, "rgb or rgba");
        if (kept) reinterpret_cast<float4*>(q.fcol)[base + at] = reinterpret_cast<const float4*>(q.col)[v];
    }
}

// after k_filter_emit: firstVertex goes through vertexMap (a kept shell's vertices are kept)
__global__ void __launch_bounds__(kMeshBlock) k_filter_shells(FilterParams q) {
    __shared__ uint32_t sWave[kMeshWaves];
    const uint32_t s = blockIdx.x * kMeshBlock + threadIdx.x;
    const bool kept = shell_kept(q, s);
    uint32_t n;
    const uint32_t at = block_rank(kept, sWave, &n);
    if (s < q.S) {
        const uint32_t to = (uint32_t)q.shellCnt[blockIdx.x] + at;
        q.shellMap[s] = kept ? to : kDropped;
        if (kept) {
            PsShell h = q.shells[s];
            const uint32_t first = h.firstVertex < q.V ? q.vertexMap[h.firstVertex] : kDropped;
            if (first == kDropped) atomicOr(&q.ctl[cErr], 1u);
            h.firstVertex = first;
            q.fshells[to] = h;
        }
    }
    if (s == 0u) {
        const uint64_t mesh = q.blockCnt[q.blocks];
        q.ctl[cShells] = (uint32_t)q.shellCnt[q.shellBlocks];
        q.ctl[cVertices] = (uint32_t)mesh;
        q.ctl[cTriangles] = (uint32_t)(mesh >> 32);
    }
}

__global__ void __launch_bounds__(kMeshBlock) k_filter_tris(FilterParams q) {
    __shared__ __attribute__((aligned(16))) uint32_t sIn[3 * kMeshBlock];
    __shared__ uint32_t sOut[3 * kMeshBlock];
    __shared__ uint32_t sWave[kMeshWaves];
    const uint32_t t0 = blockIdx.x * kMeshBlock;
    const uint32_t t = t0 + threadIdx.x;
    const uint32_t n = min(kMeshBlock, q.T - t0);
    const bool kept = t < q.T && shell_kept(q, q.triShell[t]);
    uint32_t nKept;
    const uint32_t at = block_rank(kept, sWave, &nKept);
    if (nKept == 0u) return;  // block-uniform
    const uint32_t base = (uint32_t)(q.blockCnt[blockIdx.x] >> 32);
    stage_in(q.tris, t0, n, sIn);
    if (kept) {
        bool bad = false;
        for (uint32_t k = 0; k < 3u; ++k) {
            const uint32_t c = sIn[3u * threadIdx.x + k];
            // a kept triangle's corners are kept: its shell is theirs
            const uint32_t m = c < q.V ? q.vertexMap[c] : kDropped;
            bad |= m == kDropped;
            sOut[3u * at + k] = m;
        }
        if (bad) atomicOr(&q.ctl[cErr], 1u);
    }
    stage_out(q.ftris, base, nKept, sOut);
}

const char* kFilterPhaseNames[kFilterPhases] = {"filter total",  "mask upload + k_filter_select", "k_filter_flags",
                                                "k_weld_scan x 2", "k_filter_emit",               "k_filter_shells",
                                                "k_filter_tris"};

}  // namespace

int filter_run(WeldState& W, hipStream_t s, bool timed, const PsShellFilter* f, const uint8_t* mask, uint32_t maskCount,
               PsFilterInfo* info) {
    FilterState& F = W.filter;
    if (!W.shells.valid) return PSGPU_RET_PARAM_ERROR;
    const uint32_t V = W.shells.info.ctVertices, T = W.shells.info.ctTriangles, S = W.shells.info.ctShells;
    FilterParams q;
    memset(&q, 0, sizeof(q));
    // a call refused for its arguments leaves an earlier result as it was
    if (!filter_criteria(f, &q.crit) || !filter_mask_fits(mask, maskCount, S)) return PSGPU_RET_PARAM_ERROR;
    F.valid = false;
    memset(&F.info, 0, sizeof(F.info));
    F.times.clear();
    F.info.ctInputVertices = V;
    F.info.ctInputTriangles = T;
    F.info.ctInputShells = S;
    if (S == 0) {  // an empty weld: nothing to launch
        F.valid = true;
        if (info) *info = F.info;
        return PSGPU_RET_SUCCESS;
    }
    const uint32_t shellBlocks = mesh_blocks(S), blocks = mesh_blocks(std::max(V, T));
    constexpr Growth H = Growth::ByHalf;
    PSGPU_CHECK(F.mask.reserve((size_t)S, H));
    PSGPU_CHECK(F.keep.reserve((size_t)S, H));
    PSGPU_CHECK(F.shellCnt.reserve((size_t)shellBlocks + 1, H));
    PSGPU_CHECK(F.blockCnt.reserve((size_t)blocks + 1, H));
    PSGPU_CHECK(F.ctl.reserve((size_t)kCtlWords, H));
    PSGPU_CHECK(F.pos.reserve((size_t)V * 3, H));
    PSGPU_CHECK(F.nrm.reserve((size_t)V * 3, H));
    PSGPU_CHECK(F.col.reserve((size_t)V * W.colW, H));
    PSGPU_CHECK(F.tris.reserve((size_t)T * 3, H));
    PSGPU_CHECK(F.vertexMap.reserve((size_t)V, H));
    PSGPU_CHECK(F.shellMap.reserve((size_t)S, H));
    PSGPU_CHECK(F.shells.reserve((size_t)S, H));
    q.pos = W.pos;
    q.nrm = W.nrm;
    q.col = W.col;
    q.tris = W.tris;
    q.shells = W.shells.shells;
    q.vertexShell = W.shells.vertexShell;
    q.triShell = W.shells.triShell;
    q.V = V;
    q.T = T;
    q.S = S;
    q.mask = mask ? F.mask.ptr : nullptr;
    q.keep = F.keep;
    q.shellCnt = F.shellCnt;
    q.blockCnt = F.blockCnt;
    q.shellBlocks = shellBlocks;
    q.blocks = blocks;
    q.ctl = F.ctl;
    q.fpos = F.pos;
    q.fnrm = F.nrm;
    q.fcol = F.col;
    q.ftris = F.tris;
    q.vertexMap = F.vertexMap;
    q.shellMap = F.shellMap;
    q.fshells = F.shells;
    PSGPU_CHECK(F.times.begin(timed));
    auto mark = [&]() { return F.times.mark(s); };
    const dim3 blk(kMeshBlock);
    PSGPU_CHECK(mark());
    if (mask) PSGPU_CHECK(hipMemcpyAsync(F.mask, mask, (size_t)S, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_filter_select, dim3(shellBlocks), blk, 0, s, q);
    PSGPU_CHECK(mark());
    hipLaunchKernelGGL(k_filter_flags, dim3(blocks), blk, 0, s, q);
    PSGPU_CHECK(mark());
    weld_scan_blocks(F.shellCnt, shellBlocks, s);
    weld_scan_blocks(F.blockCnt, blocks, s);
    PSGPU_CHECK(mark());
    if (W.colW == 4)
        hipLaunchKernelGGL(k_filter_emit<4>, dim3(mesh_blocks(V)), blk, 0, s, q);
    else
        hipLaunchKernelGGL(k_filter_emit<3>, dim3(mesh_blocks(V)), blk, 0, s, q);
    PSGPU_CHECK(mark());
    hipLaunchKernelGGL(k_filter_shells, dim3(shellBlocks), blk, 0, s, q);
    PSGPU_CHECK(mark());
    if (T) hipLaunchKernelGGL(k_filter_tris, dim3(mesh_blocks(T)), blk, 0, s, q);
    PSGPU_CHECK(mark());
    PSGPU_CHECK(hipGetLastError());
    uint32_t ctl[kCtlWords] = {};
    PSGPU_CHECK(hipMemcpyAsync(ctl, F.ctl, sizeof(ctl), hipMemcpyDeviceToHost, s));
    PSGPU_CHECK(hipStreamSynchronize(s));
    if (ctl[cErr] || ctl[cShells] > S || ctl[cVertices] > V || ctl[cTriangles] > T) return PSGPU_RET_DEVICE_ERROR;
    F.times.collect();
    F.info.ctShells = ctl[cShells];
    F.info.ctVertices = ctl[cVertices];
    F.info.ctTriangles = ctl[cTriangles];
    F.valid = true;
    if (info) *info = F.info;
    return PSGPU_RET_SUCCESS;
}

int filter_device(const WeldState& W, PsFilterDevice* out) {
    const FilterState& F = W.filter;
    if (!out || !W.shells.valid || !F.valid) return PSGPU_RET_PARAM_ERROR;
    const bool any = F.info.ctInputShells != 0;  // an empty weld has no arrays
    out->pos = any ? F.pos.ptr : nullptr;
    out->nrm = any ? F.nrm.ptr : nullptr;
    out->col = any ? F.col.ptr : nullptr;
    out->tris = any ? F.tris.ptr : nullptr;
    out->vertexMap = any ? F.vertexMap.ptr : nullptr;
    out->shellMap = any ? F.shellMap.ptr : nullptr;
    out->shells = any ? F.shells.ptr : nullptr;
    return PSGPU_RET_SUCCESS;
}

int filter_download(const WeldState& W, float* pos, float* nrm, float* col, uint32_t* tris, uint32_t* vertexMap,
                    uint32_t* shellMap, PsShell* shells, uint32_t shellCapacity) {
    const FilterState& F = W.filter;
    if (!W.shells.valid || !F.valid) return PSGPU_RET_PARAM_ERROR;
    const PsFilterInfo& I = F.info;
    const size_t V = I.ctVertices, T = I.ctTriangles, S = I.ctShells;
    if (shells && shellCapacity < S) return PSGPU_RET_PARAM_ERROR;
    PSGPU_CHECK(download_if(pos, F.pos, V, 12));
    PSGPU_CHECK(download_if(nrm, F.nrm, V, 12));
    PSGPU_CHECK(download_if(col, F.col, V, 4 * W.colW));
    PSGPU_CHECK(download_if(tris, F.tris, T, 12));
    PSGPU_CHECK(download_if(vertexMap, F.vertexMap, I.ctInputVertices, 4));
    PSGPU_CHECK(download_if(shellMap, F.shellMap, I.ctInputShells, 4));
    PSGPU_CHECK(download_if(shells, F.shells, S, sizeof(PsShell)));
    return PSGPU_RET_SUCCESS;
}

int filter_times(const WeldState& W, float* ms, int maxPhases, const char** names) {
    return W.filter.times.report(ms, maxPhases, names, kFilterPhaseNames);
}

}  // namespace psgpu

using namespace psgpu;

extern "C" {

int psgpu_weld_filter(psgpu_ctx* c, const PsShellFilter* f, const uint8_t* mask, uint32_t maskCount,
                      PsFilterInfo* info) {
    if (!ctx_welded(c)) return PSGPU_RET_PARAM_ERROR;
    const int rc = set_device(c);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    return filter_run(c->weld, c->stream, c->timing != 0, f, mask, maskCount, info);
}

int psgpu_weld_filter_device(psgpu_ctx* c, PsFilterDevice* out) {
    if (!ctx_welded(c)) return PSGPU_RET_PARAM_ERROR;
    return filter_device(c->weld, out);
}

int psgpu_download_weld_filter(psgpu_ctx* c, float* pos, float* nrm, float* col, uint32_t* tris, uint32_t* vertexMap,
                               uint32_t* shellMap, PsShell* shells, uint32_t shellCapacity) {
    if (!ctx_welded(c)) return PSGPU_RET_PARAM_ERROR;
    const int rc = set_device(c);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    return filter_download(c->weld, pos, nrm, col, tris, vertexMap, shellMap, shells, shellCapacity);
}

int psgpu_weld_filter_times(psgpu_ctx* c, float* ms, int maxPhases, const char** names) {
    return c ? filter_times(c->weld, ms, maxPhases, names) : 0;
}

}  // extern "C"
