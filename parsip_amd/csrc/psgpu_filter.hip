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
//   k_filter_emit    one lane per welded vertex: vertexMap (wave ballot prefix + block base),
//                    the kept pos / nrm / col staged through LDS (16-byte loads, consecutive
//                    stores), as k_weld_emit does
//   k_filter_shells  one lane per shell: shellMap, the kept PsShell records with firstVertex
//                    through vertexMap; the totals into the control words
//   k_filter_tris    one lane per triangle: the kept ones compacted in order as vertexMap[tris],
//                    staged through LDS the same way
//
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

namespace psgpu {

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kWaves = kBlock / 64;
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
    uint64_t* shellCnt;   // shellBlocks + 1: kept shells per block of kBlock shells, then scanned
    uint64_t* blockCnt;   // blocks + 1: kept vertices | kept triangles << 32 per block, then scanned
    uint32_t shellBlocks, blocks;
    uint32_t* ctl;
    float *fpos, *fnrm, *fcol;  // the filtered mesh
    uint32_t* ftris;
    uint32_t* vertexMap;
    uint32_t* shellMap;
    PsShell* fshells;
};

// this lane's place among the block's lanes with the flag set; *total: how many have it.
// Every lane of the block calls this.
__device__ __forceinline__ uint32_t block_excl_count(bool flag, uint32_t* sWave, uint32_t* total) {
    const uint64_t b = __ballot(flag);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t at = (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
    __syncthreads();  // sWave may still be read from an earlier call
    if (lane == 0u) sWave[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    uint32_t n = 0;
    for (uint32_t w = 0; w < kWaves; ++w) {
        if (w < wave) at += sWave[w];
        n += sWave[w];
    }
    *total = n;
    return at;
}

__device__ __forceinline__ bool shell_kept(const FilterParams& q, uint32_t s) { return s < q.S && q.keep[s] != 0; }

__global__ void __launch_bounds__(kBlock) k_filter_select(FilterParams q) {
    __shared__ uint32_t sWave[kWaves];
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
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
    (void)block_excl_count(keep, sWave, &n);
    if (threadIdx.x == 0) q.shellCnt[blockIdx.x] = n;
    if (s == 0u) q.ctl[cErr] = 0u;
}

__global__ void __launch_bounds__(kBlock) k_filter_flags(FilterParams q) {
    __shared__ uint32_t sWave[kWaves];
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const bool v = i < q.V && shell_kept(q, q.vertexShell[i]);
    const bool t = i < q.T && shell_kept(q, q.triShell[i]);
    uint32_t nv, nt;
    (void)block_excl_count(v, sWave, &nv);
    (void)block_excl_count(t, sWave, &nt);
    if (threadIdx.x == 0) q.blockCnt[blockIdx.x] = (uint64_t)nv | (uint64_t)nt << 32;
}

// Three words an element (a vertex attribute, a triangle's corners) of the block's elements
// [i0, i0 + n): 16-byte loads into LDS.  i0 is a multiple of kBlock, so src + 3 i0 is 16-byte
// aligned.
__device__ __forceinline__ void stage_in(const uint32_t* __restrict__ src, uint32_t i0, uint32_t n, uint32_t* sIn) {
    const uint32_t words = 3u * n;
    const uint32_t* s = src + (size_t)i0 * 3u;
    for (uint32_t x = threadIdx.x * 4u; x < words; x += kBlock * 4u) {
        if (x + 4u <= words) {
            *reinterpret_cast<uint4*>(sIn + x) = *reinterpret_cast<const uint4*>(s + x);
        } else {
            for (uint32_t y = x; y < words; ++y) sIn[y] = s[y];
        }
    }
    __syncthreads();
}

// the block's nKept compacted elements in sOut as consecutive words from element `base` of dst
__device__ __forceinline__ void stage_out(uint32_t* __restrict__ dst, uint32_t base, uint32_t nKept, const uint32_t* sOut) {
    __syncthreads();
    uint32_t* d = dst + (size_t)base * 3u;
    for (uint32_t x = threadIdx.x; x < 3u * nKept; x += kBlock) d[x] = sOut[x];
    __syncthreads();
}

// one attribute array: the kept vertices' words, bit for bit
__device__ __forceinline__ void filter_copy(const float* src, float* dst, uint32_t v0, uint32_t n, bool kept,
                                            uint32_t at, uint32_t nKept, uint32_t base, uint32_t* sIn, uint32_t* sOut) {
    stage_in(reinterpret_cast<const uint32_t*>(src), v0, n, sIn);
    if (kept) {
        sOut[3u * at] = sIn[3u * threadIdx.x];
        sOut[3u * at + 1u] = sIn[3u * threadIdx.x + 1u];
        sOut[3u * at + 2u] = sIn[3u * threadIdx.x + 2u];
    }
    stage_out(reinterpret_cast<uint32_t*>(dst), base, nKept, sOut);
}

__global__ void __launch_bounds__(kBlock) k_filter_emit(FilterParams q) {
    __shared__ __attribute__((aligned(16))) uint32_t sIn[3 * kBlock];
    __shared__ uint32_t sOut[3 * kBlock];
    __shared__ uint32_t sWave[kWaves];
    const uint32_t v0 = blockIdx.x * kBlock;
    const uint32_t v = v0 + threadIdx.x;
    const uint32_t n = min(kBlock, q.V - v0);
    const bool kept = v < q.V && shell_kept(q, q.vertexShell[v]);
    uint32_t nKept;
    const uint32_t at = block_excl_count(kept, sWave, &nKept);
    const uint32_t base = (uint32_t)q.blockCnt[blockIdx.x];
    if (v < q.V) q.vertexMap[v] = kept ? base + at : kDropped;
    if (nKept == 0u) return;  // block-uniform
    filter_copy(q.pos, q.fpos, v0, n, kept, at, nKept, base, sIn, sOut);
    filter_copy(q.nrm, q.fnrm, v0, n, kept, at, nKept, base, sIn, sOut);
    filter_copy(q.col, q.fcol, v0, n, kept, at, nKept, base, sIn, sOut);
}

// after k_filter_emit: firstVertex goes through vertexMap (a kept shell's vertices are kept)
__global__ void __launch_bounds__(kBlock) k_filter_shells(FilterParams q) {
    __shared__ uint32_t sWave[kWaves];
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    const bool kept = shell_kept(q, s);
    uint32_t n;
    const uint32_t at = block_excl_count(kept, sWave, &n);
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

__global__ void __launch_bounds__(kBlock) k_filter_tris(FilterParams q) {
    __shared__ __attribute__((aligned(16))) uint32_t sIn[3 * kBlock];
    __shared__ uint32_t sOut[3 * kBlock];
    __shared__ uint32_t sWave[kWaves];
    const uint32_t t0 = blockIdx.x * kBlock;
    const uint32_t t = t0 + threadIdx.x;
    const uint32_t n = min(kBlock, q.T - t0);
    const bool kept = t < q.T && shell_kept(q, q.triShell[t]);
    uint32_t nKept;
    const uint32_t at = block_excl_count(kept, sWave, &nKept);
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

inline uint32_t blocks_of(uint64_t n) { return (uint32_t)((n + kBlock - 1) / kBlock); }

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
    for (float& ms : F.lastMs) ms = 0.0f;
    F.info.ctInputVertices = V;
    F.info.ctInputTriangles = T;
    F.info.ctInputShells = S;
    if (S == 0) {  // an empty weld: nothing to launch
        F.valid = true;
        if (info) *info = F.info;
        return PSGPU_RET_SUCCESS;
    }
    const uint32_t shellBlocks = blocks_of(S), blocks = blocks_of(std::max(V, T));
    constexpr Growth H = Growth::ByHalf;
    PSGPU_CHECK(F.mask.reserve((size_t)S, H));
    PSGPU_CHECK(F.keep.reserve((size_t)S, H));
    PSGPU_CHECK(F.shellCnt.reserve((size_t)shellBlocks + 1, H));
    PSGPU_CHECK(F.blockCnt.reserve((size_t)blocks + 1, H));
    PSGPU_CHECK(F.ctl.reserve((size_t)kCtlWords, H));
    PSGPU_CHECK(F.pos.reserve((size_t)V * 3, H));
    PSGPU_CHECK(F.nrm.reserve((size_t)V * 3, H));
    PSGPU_CHECK(F.col.reserve((size_t)V * 3, H));
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
    if (timed)
        for (hipEvent_t& e : F.ev)
            if (!e) PSGPU_CHECK(hipEventCreate(&e));
    int phase = 0;
    auto mark = [&]() -> hipError_t { return timed ? hipEventRecord(F.ev[phase++], s) : hipSuccess; };
    const dim3 blk(kBlock);
    PSGPU_CHECK(mark());
    if (mask) PSGPU_CHECK(hipMemcpyAsync(F.mask, mask, (size_t)S, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_filter_select, dim3(shellBlocks), blk, 0, s, q);
    PSGPU_CHECK(mark());
    hipLaunchKernelGGL(k_filter_flags, dim3(blocks), blk, 0, s, q);
    PSGPU_CHECK(mark());
    weld_scan_blocks(F.shellCnt, shellBlocks, s);
    weld_scan_blocks(F.blockCnt, blocks, s);
    PSGPU_CHECK(mark());
    hipLaunchKernelGGL(k_filter_emit, dim3(blocks_of(V)), blk, 0, s, q);
    PSGPU_CHECK(mark());
    hipLaunchKernelGGL(k_filter_shells, dim3(shellBlocks), blk, 0, s, q);
    PSGPU_CHECK(mark());
    if (T) hipLaunchKernelGGL(k_filter_tris, dim3(blocks_of(T)), blk, 0, s, q);
    PSGPU_CHECK(mark());
    PSGPU_CHECK(hipGetLastError());
    uint32_t ctl[kCtlWords] = {};
    PSGPU_CHECK(hipMemcpyAsync(ctl, F.ctl, sizeof(ctl), hipMemcpyDeviceToHost, s));
    PSGPU_CHECK(hipStreamSynchronize(s));
    if (ctl[cErr] || ctl[cShells] > S || ctl[cVertices] > V || ctl[cTriangles] > T) return PSGPU_RET_DEVICE_ERROR;
    if (timed) {
        (void)hipEventElapsedTime(&F.lastMs[0], F.ev[0], F.ev[kFilterPhases - 1]);
        for (int p = 1; p < kFilterPhases; ++p) (void)hipEventElapsedTime(&F.lastMs[p], F.ev[p - 1], F.ev[p]);
    }
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
    if (pos && V) PSGPU_CHECK(hipMemcpy(pos, F.pos, V * 12, hipMemcpyDeviceToHost));
    if (nrm && V) PSGPU_CHECK(hipMemcpy(nrm, F.nrm, V * 12, hipMemcpyDeviceToHost));
    if (col && V) PSGPU_CHECK(hipMemcpy(col, F.col, V * 12, hipMemcpyDeviceToHost));
    if (tris && T) PSGPU_CHECK(hipMemcpy(tris, F.tris, T * 12, hipMemcpyDeviceToHost));
    if (vertexMap && I.ctInputVertices)
        PSGPU_CHECK(hipMemcpy(vertexMap, F.vertexMap, (size_t)I.ctInputVertices * 4, hipMemcpyDeviceToHost));
    if (shellMap && I.ctInputShells)
        PSGPU_CHECK(hipMemcpy(shellMap, F.shellMap, (size_t)I.ctInputShells * 4, hipMemcpyDeviceToHost));
    if (shells && S) PSGPU_CHECK(hipMemcpy(shells, F.shells, S * sizeof(PsShell), hipMemcpyDeviceToHost));
    return PSGPU_RET_SUCCESS;
}

int filter_times(const WeldState& W, float* ms, int maxPhases, const char** names) {
    const int n = std::min(maxPhases, kFilterPhases);
    for (int k = 0; k < n; ++k) {
        if (ms) ms[k] = W.filter.lastMs[k];
        if (names) names[k] = kFilterPhaseNames[k];
    }
    return n;
}

}  // namespace psgpu

using namespace psgpu;

namespace {
// the context's current run has been welded (psgpu_weld_device's rule)
bool ctx_welded(const psgpu_ctx* c) { return weld_run_ready(c) && c->weld.doneSeq == c->runSeq; }
}  // namespace

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
