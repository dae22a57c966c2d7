// psgpu_weld.hip — device-side weld of a finished run's mesh by lattice-edge identity
// (psgpu_weld / psgpu_weld_device / psgpu_download_weld, include/parsip_gpu.h).
//
// The compact mesh is the concatenation of per-MPU meshes: a vertex on a face shared by two
// MPUs is emitted by each of them (up to four on an edge line), and the copies' positions
// differ in the last bits for most cell sizes (each MPU computes the corner from its own
// origin), so no comparison of floats welds them.  The vertex records do: record (w, vid, key)
// is mesh vertex gi = offs[w] + vid on the global lattice edge
//     (7 i + sx, 7 j + sy, 7 k + sz, axis),  (i, j, k) = MPU w + mpuBegin in x-major order.
// Vertices with equal edges are one welded vertex; welded vertices are ordered by their
// smallest input index and take its attributes; vertexMap[gi] is the welded id.
//
//   k_weld_mark     one lane per vertex record (record_edge_id): interior records (no off-axis
//                   coordinate 0 or 7) are their own representative; seam records enter an
//                   open-addressing table (table_claim of the edge id, then a 32-bit atomicMin
//                   of gi)
//   k_weld_resolve  one lane per vertex: representative = the slot's minimum; per-block
//                   counts of kept and of seam vertices
//   k_weld_scan     one block: exclusive scan of the block counts, the totals
//   k_weld_emit     one lane per vertex: the kept vertices' welded ids (block_rank + base),
//                   their pos / nrm / col compacted through LDS (compact3: 16-byte loads,
//                   coalesced stores); k_weld_emit<4>, the compat context's rgba colours
//                   (psgpu_gui.hip): one 16-byte load and store a kept vertex
//   k_weld_map      vertexMap[gi] = id[rep[gi]] and tris = id[rep[tris]], 16 bytes a lane
//
// A group's parts (psgpu_group_weld, psgpu_group.cpp) weld in the gathered mesh's global index
// space.  The gather brings no records, so each part names its vertices' edges itself:
//
//   k_weld_edges    on the part's device, one lane per vertex record: edge[gi] = the 62-bit
//                   edge id of record_edge_id (all ones: interior); the arrays are copied
//                   behind one another on the gathering device
//   k_weld_mark_ids there, one lane per gathered vertex: k_weld_mark's table insert from the id
//
// and k_weld_resolve .. k_weld_map run on the gathered arrays as they do on a context's:
// weld_begin / weld_enqueue / weld_end below are the one launch sequence of both.  The stages
// named in brackets are psgpu_mesh_stages.h's, shared with the shells and the filter.
//
// The phases are ordered by kernel boundaries alone: no block waits for another inside a
// launch.  Every value written is a function of the records alone (the table's slot
// assignment depends on arrival order, the minimum in a slot does not), so two welds of one
// run give the same bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>

#include "psgpu_internal.h"
#include "psgpu_mesh_stages.h"

namespace psgpu {

namespace {

struct WeldParams {
    WeldRecords rec;     // k_weld_mark
    uint32_t V, T;
    uint64_t* keys;      // table: tableMask + 1 edge ids ...
    uint32_t* mins;      // ... and the smallest gi seen with each
    uint32_t tableMask;
    uint32_t* rep;       // V: the mark kernel the table slot (kNoSlot: interior), k_weld_resolve the representative
    uint32_t* kid;       // V: welded id of a kept vertex
    uint64_t* blockCnt;  // blocks + 1: kept | seam << 32 per block of kMeshBlock vertices, then scanned; [blocks] the totals
    uint32_t blocks;
    const float *pos, *nrm, *col;
    const uint32_t* tris;
    float *wpos, *wnrm, *wcol;
    uint32_t* wtris;
    uint32_t* map;
    uint32_t mapBlocks;  // k_weld_map: blocks [0, mapBlocks) write the map, the rest the triangles
};

// vertex gi on edge `id` (kEmptyKey: interior) enters the table: rep[gi] = its slot
__device__ __forceinline__ void weld_insert(const WeldParams& q, uint32_t gi, uint64_t id) {
    const uint32_t slot = id == kEmptyKey ? kNoSlot : table_claim(q.keys, q.tableMask, id);
    if (slot != kNoSlot) atomicMin(&q.mins[slot], gi);
    q.rep[gi] = slot;
}

__global__ void __launch_bounds__(kMeshBlock) k_weld_mark(WeldParams q) {
    __shared__ uint32_t sStart[kShards + 1];
    uint32_t gi;
    const uint64_t id = record_edge_id(q.rec, q.V, sStart, &gi);
    if (gi != kNoSlot) weld_insert(q, gi, id);
}

// A part's records as edge ids (psgpu_group_weld): edge[gi] (gi local to the part) instead of
// a table; the array was filled with ones, so an interior record and a missing one both read
// as kEmptyKey.
__global__ void __launch_bounds__(kMeshBlock) k_weld_edges(WeldRecords q, uint32_t V, uint64_t* edge) {
    __shared__ uint32_t sStart[kShards + 1];
    uint32_t gi;
    const uint64_t id = record_edge_id(q, V, sStart, &gi);
    if (id != kEmptyKey) edge[gi] = id;
}

// k_weld_mark over the gathered vertices' edge ids: one lane per vertex, the same insert
__global__ void __launch_bounds__(kMeshBlock) k_weld_mark_ids(WeldParams q, const uint64_t* __restrict__ edge) {
    const uint32_t gi = blockIdx.x * kMeshBlock + threadIdx.x;
    if (gi < q.V) weld_insert(q, gi, edge[gi]);
}

__global__ void __launch_bounds__(kMeshBlock) k_weld_resolve(WeldParams q) {
    __shared__ uint32_t sKept[kMeshWaves], sSeam[kMeshWaves];
    const uint32_t gi = blockIdx.x * kMeshBlock + threadIdx.x;
    bool kept = false, seam = false;
    if (gi < q.V) {
        const uint32_t slot = q.rep[gi];
        seam = slot <= q.tableMask;  // kNoSlot: interior
        uint32_t rep = seam ? q.mins[slot] : gi;
        if (rep >= q.V) rep = gi;
        q.rep[gi] = rep;
        kept = rep == gi;
    }
    const uint32_t ak = wave_rank(kept, sKept), as = wave_rank(seam, sSeam);
    __syncthreads();
    uint32_t nk, ns;
    (void)block_rank_sum(ak, sKept, &nk);
    (void)block_rank_sum(as, sSeam, &ns);
    if (threadIdx.x == 0) q.blockCnt[blockIdx.x] = (uint64_t)nk | (uint64_t)ns << 32;
}

// one block: blockCnt[0..blocks) becomes its exclusive scan, blockCnt[blocks] the totals
// (both halves of a word stay below 2^32: they count vertices); also the shells' and the
// filter's scan (weld_scan_blocks)
__global__ void __launch_bounds__(kMeshBlock) k_weld_scan(uint64_t* blockCnt, uint32_t blocks) {
    __shared__ uint64_t sWave[kMeshWaves];
    __shared__ uint64_t sCarry;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) sCarry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < blocks; base += kMeshBlock) {
        const uint32_t b = base + threadIdx.x;
        const uint64_t v = b < blocks ? blockCnt[b] : 0ull;
        uint64_t incl = v;
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint64_t up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63u) sWave[wave] = incl;
        __syncthreads();
        uint64_t before = sCarry;
        for (uint32_t w = 0; w < wave; ++w) before += sWave[w];
        if (b < blocks) blockCnt[b] = before + incl - v;
        __syncthreads();
        if (threadIdx.x == kMeshBlock - 1) sCarry = before + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) blockCnt[blocks] = sCarry;
}

template <int W>  // floats a colour
__global__ void __launch_bounds__(kMeshBlock) k_weld_emit(WeldParams q) {
    __shared__ __attribute__((aligned(16))) uint32_t sIn[3 * kMeshBlock];
    __shared__ uint32_t sOut[3 * kMeshBlock];
    __shared__ uint32_t sWave[kMeshWaves];
    const uint32_t v0 = blockIdx.x * kMeshBlock;
    const uint32_t gi = v0 + threadIdx.x;
    const uint32_t n = min(kMeshBlock, q.V - v0);
    const bool kept = gi < q.V && q.rep[gi] == gi;
    uint32_t nKept;
    const uint32_t at = block_rank(kept, sWave, &nKept);
    const uint32_t base = (uint32_t)q.blockCnt[blockIdx.x];
    if (kept) q.kid[gi] = base + at;
    compact3(q.pos, q.wpos, v0, n, kept, at, nKept, base, sIn, sOut);
    compact3(q.nrm, q.wnrm, v0, n, kept, at, nKept, base, sIn, sOut);
    if constexpr (W == 3) {
        compact3(q.col, q.wcol, v0, n, kept, at, nKept, base, sIn, sOut);
    } else {
        static_assert(W == 4, "rgb or rgba");
        if (kept) reinterpret_cast<float4*>(q.wcol)[base + at] = reinterpret_cast<const float4*>(q.col)[gi];
    }
}

__device__ __forceinline__ uint32_t weld_id(const WeldParams& q, uint32_t v) {
    return v < q.V ? q.kid[q.rep[v]] : v;
}
__device__ __forceinline__ uint4 weld_id4(const WeldParams& q, uint4 v) {
    return make_uint4(weld_id(q, v.x), weld_id(q, v.y), weld_id(q, v.z), weld_id(q, v.w));
}

__global__ void __launch_bounds__(kMeshBlock) k_weld_map(WeldParams q) {
    if (blockIdx.x < q.mapBlocks) {  // vertexMap: 4 vertices a lane
        const uint32_t x = (blockIdx.x * kMeshBlock + threadIdx.x) * 4u;
        if (x + 4u <= q.V) {
            const uint4 r = *reinterpret_cast<const uint4*>(q.rep + x);
            *reinterpret_cast<uint4*>(q.map + x) = make_uint4(q.kid[r.x], q.kid[r.y], q.kid[r.z], q.kid[r.w]);
        } else {
            for (uint32_t y = x; y < q.V; ++y) q.map[y] = q.kid[q.rep[y]];
        }
        return;
    }
    // triangles: 4 a lane (12 indices, three 16-byte words)
    const uint64_t words = 3ull * q.T;
    const uint64_t x = ((uint64_t)(blockIdx.x - q.mapBlocks) * kMeshBlock + threadIdx.x) * 12ull;
    if (x + 12ull <= words) {
        const uint4* s = reinterpret_cast<const uint4*>(q.tris + x);
        uint4* d = reinterpret_cast<uint4*>(q.wtris + x);
        const uint4 a = s[0], b = s[1], c = s[2];
        d[0] = weld_id4(q, a);
        d[1] = weld_id4(q, b);
        d[2] = weld_id4(q, c);
    } else {
        for (uint64_t y = x; y < words; ++y) q.wtris[y] = weld_id(q, q.tris[y]);
    }
}

const char* kWeldPhaseNames[kWeldPhases] = {"weld total", "table fill + k_weld_mark", "k_weld_resolve", "k_weld_scan",
                                            "k_weld_emit", "k_weld_map"};

// The run's vertex records: one per vertex, every shard within its capacity (finish re-runs
// until they fit); shardV from the run's host counters.
int weld_records(const psgpu_ctx* c, uint32_t V, WeldRecords& r) {
    uint64_t recs = 0;
    for (int k = 0; k < kShards; ++k) {
        r.shardV[k] = c->hostCtr->shard[k].v;
        if (r.shardV[k] > c->vShardCap) return PSGPU_RET_DEVICE_ERROR;
        recs += r.shardV[k];
    }
    r.vk = c->vk;
    r.offs = c->offs;
    r.vShardCap = c->vShardCap;
    for (int a = 0; a < 3; ++a) r.dims[a] = c->dims[a];
    r.mpuBegin = c->mpuBegin;
    r.mpuCount = c->mpuCount;
    return recs == V ? PSGPU_RET_SUCCESS : PSGPU_RET_DEVICE_ERROR;
}

// Sizes the table for V > 0 input vertices, grows W's buffers to V vertices and T triangles and
// points q at them (the table, rep / kid / blockCnt / map, the welded arrays, the grid sizes).
int weld_prepare(WeldState& W, uint32_t V, uint32_t T, WeldParams& q, uint32_t* slotsOut) {
    // at most V seam records: a table of >= 2 V slots stays at most half full
    uint32_t slots = 1024;
    while (slots < 2ull * V && slots < (1u << 31)) slots <<= 1;
    const uint32_t blocks = mesh_blocks(V);
    constexpr Growth H = Growth::ByHalf;
    PSGPU_CHECK(W.table.reserve((size_t)slots * 12, H));
    PSGPU_CHECK(W.rep.reserve((size_t)V + 4, H));
    PSGPU_CHECK(W.kid.reserve((size_t)V + 4, H));
    PSGPU_CHECK(W.map.reserve((size_t)V + 4, H));
    PSGPU_CHECK(W.blockCnt.reserve((size_t)blocks + 1, H));
    PSGPU_CHECK(W.pos.reserve((size_t)V * 3, H));
    PSGPU_CHECK(W.nrm.reserve((size_t)V * 3, H));
    PSGPU_CHECK(W.col.reserve((size_t)V * W.colW, H));
    PSGPU_CHECK(W.tris.reserve((size_t)T * 3 + 4, H));
    q.V = V;
    q.T = T;
    q.keys = reinterpret_cast<uint64_t*>(W.table.ptr);
    q.mins = reinterpret_cast<uint32_t*>(W.table + (size_t)slots * 8);
    q.tableMask = slots - 1u;
    q.rep = W.rep;
    q.kid = W.kid;
    q.blockCnt = W.blockCnt;
    q.blocks = blocks;
    q.wpos = W.pos;
    q.wnrm = W.nrm;
    q.wcol = W.col;
    q.wtris = W.tris;
    q.map = W.map;
    q.mapBlocks = (V + 4u * kMeshBlock - 1u) / (4u * kMeshBlock);
    *slotsOut = slots;
    return PSGPU_RET_SUCCESS;
}

}  // namespace

// the current run is finished, uncollected by nothing newer, and whole
bool weld_run_ready(const psgpu_ctx* c) {
    return c && !c->pending && c->haveResult && c->finishedSeq == c->runSeq;
}

bool weld_lattice_fits(const uint32_t* dims) {
    for (int a = 0; a < 3; ++a)
        if (7ull * dims[a] >= (1ull << kCoordBits)) return false;
    return true;
}

void weld_state_free(WeldState& W) {
    W.filter.times.free();
    W.shells.times.free();
    W.times.free();
    W = WeldState{};  // releases the weld's buffers, the shells' and the filter's
}

void weld_scan_blocks(uint64_t* blockCnt, uint32_t blocks, hipStream_t s) {
    hipLaunchKernelGGL(k_weld_scan, dim3(1), dim3(kMeshBlock), 0, s, blockCnt, blocks);
}

int weld_edges(psgpu_ctx* c, uint64_t* edge, hipStream_t s) {
    const uint32_t V = c->info.ctVertices;
    if (V == 0) return PSGPU_RET_SUCCESS;
    WeldRecords r;
    const int rc = weld_records(c, V, r);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    PSGPU_CHECK(hipMemsetAsync(edge, 0xff, (size_t)V * 8, s));
    hipLaunchKernelGGL(k_weld_edges, dim3(mesh_blocks(V)), dim3(kMeshBlock), 0, s, r, V, edge);
    PSGPU_CHECK(hipGetLastError());
    return PSGPU_RET_SUCCESS;
}

int weld_device(const WeldState& W, PsWeldDevice* out) {
    out->pos = W.pos;
    out->nrm = W.nrm;
    out->col = W.col;
    out->tris = W.tris;
    out->vertexMap = W.map;
    return PSGPU_RET_SUCCESS;
}

int weld_download(const WeldState& W, float* pos, float* nrm, float* col, uint32_t* tris, uint32_t* vertexMap) {
    const size_t V = W.info.ctVertices, T = W.info.ctTriangles, Vin = W.info.ctInputVertices;
    PSGPU_CHECK(download_if(pos, W.pos, V, 12));
    PSGPU_CHECK(download_if(nrm, W.nrm, V, 12));
    PSGPU_CHECK(download_if(col, W.col, V, 4 * W.colW));
    PSGPU_CHECK(download_if(tris, W.tris, T, 12));
    PSGPU_CHECK(download_if(vertexMap, W.map, Vin, 4));
    return PSGPU_RET_SUCCESS;
}

int weld_times(const WeldState& W, float* ms, int maxPhases, const char** names) {
    return W.times.report(ms, maxPhases, names, kWeldPhaseNames);
}

bool weld_begin(WeldState& W, uint32_t V, uint32_t T, uint64_t seq, PsWeldInfo* info) {
    W.doneSeq = ~0ull;
    W.shells.valid = false;
    W.filter.valid = false;
    memset(&W.info, 0, sizeof(W.info));
    W.info.ctInputVertices = V;
    W.info.ctTriangles = T;
    W.times.clear();
    if (V) return true;
    W.doneSeq = seq;  // an empty mesh welds to an empty mesh
    if (info) *info = W.info;
    return false;
}

int weld_enqueue(WeldState& W, const WeldInput& in, hipStream_t s, PhaseCursor marks) {
    WeldParams q;
    memset(&q, 0, sizeof(q));
    int rc = in.records ? weld_records(in.records, in.V, q.rec) : PSGPU_RET_SUCCESS;
    if (rc != PSGPU_RET_SUCCESS) return rc;
    uint32_t slots = 0;
    rc = weld_prepare(W, in.V, in.T, q, &slots);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    q.pos = in.pos;
    q.nrm = in.nrm;
    q.col = in.col;
    q.tris = in.tris;
    const dim3 blk(kMeshBlock);
    const uint32_t triBlocks = mesh_blocks(((uint64_t)q.T + 3u) / 4u);  // k_weld_map: 4 triangles a lane
    PSGPU_CHECK(marks.mark(s));
    // every key empty (all ones), every minimum 0xffffffff
    PSGPU_CHECK(hipMemsetAsync(W.table, 0xff, (size_t)slots * 12, s));
    if (in.records)
        hipLaunchKernelGGL(k_weld_mark, dim3(q.blocks), blk, 0, s, q);
    else
        hipLaunchKernelGGL(k_weld_mark_ids, dim3(q.blocks), blk, 0, s, q, in.edge);
    PSGPU_CHECK(marks.mark(s));
    hipLaunchKernelGGL(k_weld_resolve, dim3(q.blocks), blk, 0, s, q);
    PSGPU_CHECK(marks.mark(s));
    hipLaunchKernelGGL(k_weld_scan, dim3(1), blk, 0, s, q.blockCnt, q.blocks);
    PSGPU_CHECK(marks.mark(s));
    if (W.colW == 4)
        hipLaunchKernelGGL(k_weld_emit<4>, dim3(q.blocks), blk, 0, s, q);
    else
        hipLaunchKernelGGL(k_weld_emit<3>, dim3(q.blocks), blk, 0, s, q);
    PSGPU_CHECK(marks.mark(s));
    hipLaunchKernelGGL(k_weld_map, dim3(q.mapBlocks + triBlocks), blk, 0, s, q);
    PSGPU_CHECK(marks.mark(s));
    PSGPU_CHECK(hipGetLastError());
    return PSGPU_RET_SUCCESS;
}

int weld_end(WeldState& W, hipStream_t s, uint64_t seq, PsWeldInfo* info) {
    uint64_t totals = 0;  // welded | seam << 32, behind the scanned block counts
    PSGPU_CHECK(hipMemcpyAsync(&totals, W.blockCnt + mesh_blocks(W.info.ctInputVertices), sizeof(totals),
                               hipMemcpyDeviceToHost, s));
    PSGPU_CHECK(hipStreamSynchronize(s));
    W.info.ctVertices = (uint32_t)totals;
    W.info.ctSeamVertices = (uint32_t)(totals >> 32);
    W.doneSeq = seq;
    if (info) *info = W.info;
    return PSGPU_RET_SUCCESS;
}

}  // namespace psgpu

using namespace psgpu;

extern "C" {

int psgpu_weld(psgpu_ctx* c, PsWeldInfo* info) {
    if (!weld_run_ready(c)) return PSGPU_RET_PARAM_ERROR;
    if (c->info.firstOverflowMPU >= 0) return PSGPU_RET_PARAM_ERROR;  // past the reference's 512 per MPU (records complete)
    if (!weld_lattice_fits(c->dims)) return PSGPU_RET_PARAM_ERROR;
    int rc = set_device(c);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    WeldState& W = c->weld;
    const WeldInput in{c->pos, c->nrm, c->col, c->tris, c->info.ctVertices, c->info.ctTriangles, nullptr, c};
    if (!weld_begin(W, in.V, in.T, c->runSeq, info)) return PSGPU_RET_SUCCESS;
    PSGPU_CHECK(W.times.begin(c->timing != 0));
    rc = weld_enqueue(W, in, c->stream, W.times.rest());
    if (rc == PSGPU_RET_SUCCESS) rc = weld_end(W, c->stream, c->runSeq, info);
    if (rc == PSGPU_RET_SUCCESS) W.times.collect();
    return rc;
}

int psgpu_weld_device(psgpu_ctx* c, PsWeldDevice* out) {
    if (!out || !ctx_welded(c)) return PSGPU_RET_PARAM_ERROR;
    return weld_device(c->weld, out);
}

int psgpu_download_weld(psgpu_ctx* c, float* pos, float* nrm, float* col, uint32_t* tris, uint32_t* vertexMap) {
    if (!ctx_welded(c)) return PSGPU_RET_PARAM_ERROR;
    const int rc = set_device(c);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    return weld_download(c->weld, pos, nrm, col, tris, vertexMap);
}

int psgpu_weld_times(psgpu_ctx* c, float* ms, int maxPhases, const char** names) {
    return c ? weld_times(c->weld, ms, maxPhases, names) : 0;
}

}  // extern "C"
