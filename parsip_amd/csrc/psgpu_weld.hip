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
//   k_weld_mark     one lane per vertex record: interior records (no off-axis coordinate 0
//                   or 7) are their own representative; seam records enter an open-addressing
//                   table (64-bit CAS on the edge id, then a 32-bit atomicMin of gi)
//   k_weld_resolve  one lane per vertex: representative = the slot's minimum; per-block
//                   counts of kept and of seam vertices
//   k_weld_scan     one block: exclusive scan of the block counts, the totals
//   k_weld_emit     one lane per vertex: the kept vertices' welded ids (block scan + base),
//                   their pos / nrm / col staged through LDS (16-byte loads, coalesced stores)
//   k_weld_map      vertexMap[gi] = id[rep[gi]] and tris = id[rep[tris]], 16 bytes a lane
//
// A group's parts (psgpu_group_weld, psgpu_group.cpp) weld in the gathered mesh's global index
// space.  The gather brings no records, so each part names its vertices' edges itself:
//
//   k_weld_edges    on the part's device, one lane per vertex record: edge[gi] = the 62-bit
//                   edge id k_weld_mark composes (all ones: interior); the arrays are copied
//                   behind one another on the gathering device
//   k_weld_mark_ids there, one lane per gathered vertex: k_weld_mark's table insert from the id
//
// and k_weld_resolve .. k_weld_map run on the gathered arrays as they do on a context's.
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

namespace psgpu {

namespace {

constexpr uint32_t kWeldBlock = 256;
constexpr uint32_t kNoSlot = 0xffffffffu;
constexpr uint64_t kEmptyKey = ~0ull;  // no edge id: ids use 62 bits
constexpr uint32_t kCoordBits = 20;    // per lattice coordinate of the edge id (psgpu_weld checks the lattice)

struct WeldParams {
    const VertexKey* vk;
    const uint64_t* offs;
    uint32_t vShardCap;
    uint32_t shardV[kShards];  // vertex records per shard (the run's host counters)
    uint32_t dims[3];
    uint32_t mpuBegin, mpuCount;
    uint32_t V, T;
    uint64_t* keys;      // table: tableMask + 1 edge ids ...
    uint32_t* mins;      // ... and the smallest gi seen with each
    uint32_t tableMask;
    uint32_t* rep;       // V: k_weld_mark the table slot (kNoSlot: interior), k_weld_resolve the representative
    uint32_t* kid;       // V: welded id of a kept vertex
    uint64_t* blockCnt;  // blocks + 1: kept | seam << 32 per block of kWeldBlock vertices, then scanned; [blocks] the totals
    uint32_t blocks;
    const float *pos, *nrm, *col;
    const uint32_t* tris;
    float *wpos, *wnrm, *wcol;
    uint32_t* wtris;
    uint32_t* map;
    uint32_t mapBlocks;  // k_weld_map: blocks [0, mapBlocks) write the map, the rest the triangles
};

__device__ __forceinline__ uint32_t weld_hash(uint64_t x) {  // murmur3's 64-bit finaliser
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return (uint32_t)x;
}

__global__ void __launch_bounds__(kWeldBlock) k_weld_mark(WeldParams q) {
    __shared__ uint32_t sStart[kShards + 1];
    if (threadIdx.x == 0) {
        uint32_t at = 0;
        for (int k = 0; k < kShards; ++k) {
            sStart[k] = at;
            at += q.shardV[k];
        }
        sStart[kShards] = at;
    }
    __syncthreads();
    const uint32_t r = blockIdx.x * kWeldBlock + threadIdx.x;
    if (r >= sStart[kShards]) return;
    uint32_t shard = 0;  // the last shard whose first record is <= r
    for (uint32_t step = kShards / 2; step; step >>= 1)
        if (sStart[shard + step] <= r) shard += step;
    const VertexKey K = q.vk[(size_t)shard * q.vShardCap + (r - sStart[shard])];
    if (K.w >= q.mpuCount) return;
    const uint32_t gi = (uint32_t)q.offs[K.w] + (K.vidKey & 0xffffu);
    if (gi >= q.V) return;
    const uint32_t key = K.vidKey >> 16;
    const uint32_t sx = key & 7u, sy = (key >> 3) & 7u, sz = (key >> 6) & 7u, ax = (key >> 9) & 3u;
    // on an MPU face: an off-axis coordinate on the MPU's first or last corner plane
    const bool fx = sx == 0u || sx == 7u, fy = sy == 0u || sy == 7u, fz = sz == 0u || sz == 7u;
    const bool seam = (ax != 0u && fx) || (ax != 1u && fy) || (ax != 2u && fz);
    if (!seam) {
        q.rep[gi] = kNoSlot;
        return;
    }
    const uint32_t m = K.w + q.mpuBegin;
    const uint32_t nyz = q.dims[1] * q.dims[2];
    const uint32_t i = m / nyz, jk = m - i * nyz;
    const uint32_t j = jk / q.dims[2], k = jk - j * q.dims[2];
    const uint64_t id = ((((uint64_t)(7u * i + sx) << kCoordBits | (uint64_t)(7u * j + sy)) << kCoordBits |
                          (uint64_t)(7u * k + sz)) << 2) | ax;
    uint32_t slot = weld_hash(id) & q.tableMask;
    // at most half the slots are ever taken (psgpu_weld sizes the table), so an empty or
    // matching slot comes up; the bound only keeps a corrupt record from spinning
    for (uint32_t tries = 0; tries <= q.tableMask; ++tries) {
        const uint64_t seen = atomicCAS((unsigned long long*)&q.keys[slot], (unsigned long long)kEmptyKey,
                                        (unsigned long long)id);
        if (seen == kEmptyKey || seen == id) {
            atomicMin(&q.mins[slot], gi);
            q.rep[gi] = slot;
            return;
        }
        slot = (slot + 1u) & q.tableMask;
    }
    q.rep[gi] = kNoSlot;
}

// A part's records as edge ids (psgpu_group_weld): k_weld_mark's shard lookup, seam test and
// id, written to edge[gi] (gi local to the part) instead of entering a table; the array was
// filled with ones, so an interior record and a missing one both read as kEmptyKey.
struct WeldEdgeParams {
    const VertexKey* vk;
    const uint64_t* offs;
    uint32_t vShardCap;
    uint32_t shardV[kShards];
    uint32_t dims[3];
    uint32_t mpuBegin, mpuCount;
    uint32_t V;
    uint64_t* edge;  // V
};

__global__ void __launch_bounds__(kWeldBlock) k_weld_edges(WeldEdgeParams q) {
    __shared__ uint32_t sStart[kShards + 1];
    if (threadIdx.x == 0) {
        uint32_t at = 0;
        for (int k = 0; k < kShards; ++k) {
            sStart[k] = at;
            at += q.shardV[k];
        }
        sStart[kShards] = at;
    }
    __syncthreads();
    const uint32_t r = blockIdx.x * kWeldBlock + threadIdx.x;
    if (r >= sStart[kShards]) return;
    uint32_t shard = 0;
    for (uint32_t step = kShards / 2; step; step >>= 1)
        if (sStart[shard + step] <= r) shard += step;
    const VertexKey K = q.vk[(size_t)shard * q.vShardCap + (r - sStart[shard])];
    if (K.w >= q.mpuCount) return;
    const uint32_t gi = (uint32_t)q.offs[K.w] + (K.vidKey & 0xffffu);
    if (gi >= q.V) return;
    const uint32_t key = K.vidKey >> 16;
    const uint32_t sx = key & 7u, sy = (key >> 3) & 7u, sz = (key >> 6) & 7u, ax = (key >> 9) & 3u;
    const bool fx = sx == 0u || sx == 7u, fy = sy == 0u || sy == 7u, fz = sz == 0u || sz == 7u;
    if (!((ax != 0u && fx) || (ax != 1u && fy) || (ax != 2u && fz))) return;  // interior: stays kEmptyKey
    const uint32_t m = K.w + q.mpuBegin;
    const uint32_t nyz = q.dims[1] * q.dims[2];
    const uint32_t i = m / nyz, jk = m - i * nyz;
    const uint32_t j = jk / q.dims[2], k = jk - j * q.dims[2];
    q.edge[gi] = ((((uint64_t)(7u * i + sx) << kCoordBits | (uint64_t)(7u * j + sy)) << kCoordBits |
                   (uint64_t)(7u * k + sz)) << 2) | ax;
}

// k_weld_mark over the gathered vertices' edge ids: one lane per vertex, the same insert
__global__ void __launch_bounds__(kWeldBlock) k_weld_mark_ids(WeldParams q, const uint64_t* __restrict__ edge) {
    const uint32_t gi = blockIdx.x * kWeldBlock + threadIdx.x;
    if (gi >= q.V) return;
    const uint64_t id = edge[gi];
    if (id == kEmptyKey) {
        q.rep[gi] = kNoSlot;
        return;
    }
    uint32_t slot = weld_hash(id) & q.tableMask;
    for (uint32_t tries = 0; tries <= q.tableMask; ++tries) {
        const uint64_t seen = atomicCAS((unsigned long long*)&q.keys[slot], (unsigned long long)kEmptyKey,
                                        (unsigned long long)id);
        if (seen == kEmptyKey || seen == id) {
            atomicMin(&q.mins[slot], gi);
            q.rep[gi] = slot;
            return;
        }
        slot = (slot + 1u) & q.tableMask;
    }
    q.rep[gi] = kNoSlot;
}

// lanes of the wave below this one with the flag set; *total: lanes of the wave with it
__device__ __forceinline__ uint32_t wave_excl_count(bool flag, uint32_t* total) {
    const uint64_t b = __ballot(flag);
    const uint32_t lane = threadIdx.x & 63u;
    *total = (uint32_t)__popcll(b);
    return (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
}

__global__ void __launch_bounds__(kWeldBlock) k_weld_resolve(WeldParams q) {
    __shared__ uint32_t sKept[kWeldBlock / 64], sSeam[kWeldBlock / 64];
    const uint32_t gi = blockIdx.x * kWeldBlock + threadIdx.x;
    bool kept = false, seam = false;
    if (gi < q.V) {
        const uint32_t slot = q.rep[gi];
        seam = slot <= q.tableMask;  // kNoSlot: interior
        uint32_t rep = seam ? q.mins[slot] : gi;
        if (rep >= q.V) rep = gi;
        q.rep[gi] = rep;
        kept = rep == gi;
    }
    uint32_t nk, ns;
    (void)wave_excl_count(kept, &nk);
    (void)wave_excl_count(seam, &ns);
    if ((threadIdx.x & 63u) == 0u) {
        sKept[threadIdx.x >> 6] = nk;
        sSeam[threadIdx.x >> 6] = ns;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t a = 0, b = 0;
        for (uint32_t w = 0; w < kWeldBlock / 64; ++w) {
            a += sKept[w];
            b += sSeam[w];
        }
        q.blockCnt[blockIdx.x] = (uint64_t)a | (uint64_t)b << 32;
    }
}

// one block: blockCnt[0..blocks) becomes its exclusive scan, blockCnt[blocks] the totals
// (both halves of a word stay below 2^32: they count vertices)
__global__ void __launch_bounds__(kWeldBlock) k_weld_scan(WeldParams q) {
    __shared__ uint64_t sWave[kWeldBlock / 64];
    __shared__ uint64_t sCarry;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) sCarry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < q.blocks; base += kWeldBlock) {
        const uint32_t b = base + threadIdx.x;
        const uint64_t v = b < q.blocks ? q.blockCnt[b] : 0ull;
        uint64_t incl = v;
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint64_t up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63u) sWave[wave] = incl;
        __syncthreads();
        uint64_t before = sCarry;
        for (uint32_t w = 0; w < wave; ++w) before += sWave[w];
        if (b < q.blocks) q.blockCnt[b] = before + incl - v;
        __syncthreads();
        if (threadIdx.x == kWeldBlock - 1) sCarry = before + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) q.blockCnt[q.blocks] = sCarry;
}

// one attribute array of the block's vertices [v0, v0 + n): 16-byte loads into LDS, the kept
// ones compacted in LDS, then stored as consecutive words from welded vertex `base`
__device__ __forceinline__ void weld_copy(const float* __restrict__ src, float* __restrict__ dst, uint32_t v0,
                                          uint32_t n, bool kept, uint32_t at, uint32_t nKept, uint32_t base,
                                          float* sIn, float* sOut) {
    const uint32_t words = 3u * n;
    const float* s = src + (size_t)v0 * 3u;  // v0 is a multiple of kWeldBlock: 16-byte aligned
    for (uint32_t x = threadIdx.x * 4u; x < words; x += kWeldBlock * 4u) {
        if (x + 4u <= words) {
            *reinterpret_cast<float4*>(sIn + x) = *reinterpret_cast<const float4*>(s + x);
        } else {
            for (uint32_t y = x; y < words; ++y) sIn[y] = s[y];
        }
    }
    __syncthreads();
    if (kept) {
        sOut[3u * at] = sIn[3u * threadIdx.x];
        sOut[3u * at + 1u] = sIn[3u * threadIdx.x + 1u];
        sOut[3u * at + 2u] = sIn[3u * threadIdx.x + 2u];
    }
    __syncthreads();
    float* d = dst + (size_t)base * 3u;
    for (uint32_t x = threadIdx.x; x < 3u * nKept; x += kWeldBlock) d[x] = sOut[x];
    __syncthreads();
}

__global__ void __launch_bounds__(kWeldBlock) k_weld_emit(WeldParams q) {
    __shared__ __attribute__((aligned(16))) float sIn[3 * kWeldBlock];
    __shared__ float sOut[3 * kWeldBlock];
    __shared__ uint32_t sWave[kWeldBlock / 64];
    const uint32_t v0 = blockIdx.x * kWeldBlock;
    const uint32_t gi = v0 + threadIdx.x;
    const uint32_t n = min(kWeldBlock, q.V - v0);
    const bool kept = gi < q.V && q.rep[gi] == gi;
    uint32_t nk;
    uint32_t at = wave_excl_count(kept, &nk);
    if ((threadIdx.x & 63u) == 0u) sWave[threadIdx.x >> 6] = nk;
    __syncthreads();
    uint32_t nKept = 0;
    for (uint32_t w = 0; w < kWeldBlock / 64; ++w) {
        if (w < (threadIdx.x >> 6)) at += sWave[w];
        nKept += sWave[w];
    }
    const uint32_t base = (uint32_t)q.blockCnt[blockIdx.x];
    if (kept) q.kid[gi] = base + at;
    weld_copy(q.pos, q.wpos, v0, n, kept, at, nKept, base, sIn, sOut);
    weld_copy(q.nrm, q.wnrm, v0, n, kept, at, nKept, base, sIn, sOut);
    weld_copy(q.col, q.wcol, v0, n, kept, at, nKept, base, sIn, sOut);
}

__device__ __forceinline__ uint32_t weld_id(const WeldParams& q, uint32_t v) {
    return v < q.V ? q.kid[q.rep[v]] : v;
}
__device__ __forceinline__ uint4 weld_id4(const WeldParams& q, uint4 v) {
    return make_uint4(weld_id(q, v.x), weld_id(q, v.y), weld_id(q, v.z), weld_id(q, v.w));
}

__global__ void __launch_bounds__(kWeldBlock) k_weld_map(WeldParams q) {
    if (blockIdx.x < q.mapBlocks) {  // vertexMap: 4 vertices a lane
        const uint32_t x = (blockIdx.x * kWeldBlock + threadIdx.x) * 4u;
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
    const uint64_t x = ((uint64_t)(blockIdx.x - q.mapBlocks) * kWeldBlock + threadIdx.x) * 12ull;
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

// the run's vertex records per shard (its host counters): one record per vertex, every shard
// within its capacity (finish re-runs until they fit)
int weld_shard_counts(const psgpu_ctx* c, uint32_t V, uint32_t* shardV) {
    uint64_t recs = 0;
    for (int k = 0; k < kShards; ++k) {
        shardV[k] = c->hostCtr->shard[k].v;
        if (shardV[k] > c->vShardCap) return PSGPU_RET_DEVICE_ERROR;
        recs += shardV[k];
    }
    return recs == V ? PSGPU_RET_SUCCESS : PSGPU_RET_DEVICE_ERROR;
}

// Sizes the table for V > 0 input vertices, grows W's buffers to V vertices and T triangles and
// points q at them (the table, rep / kid / blockCnt / map, the welded arrays, the grid sizes).
int weld_prepare(WeldState& W, uint32_t V, uint32_t T, WeldParams& q, uint32_t* slotsOut) {
    // at most V seam records: a table of >= 2 V slots stays at most half full
    uint32_t slots = 1024;
    while (slots < 2ull * V && slots < (1u << 31)) slots <<= 1;
    const uint32_t blocks = (V + kWeldBlock - 1) / kWeldBlock;
    constexpr Growth H = Growth::ByHalf;
    PSGPU_CHECK(W.table.reserve((size_t)slots * 12, H));
    PSGPU_CHECK(W.rep.reserve((size_t)V + 4, H));
    PSGPU_CHECK(W.kid.reserve((size_t)V + 4, H));
    PSGPU_CHECK(W.map.reserve((size_t)V + 4, H));
    PSGPU_CHECK(W.blockCnt.reserve((size_t)blocks + 1, H));
    PSGPU_CHECK(W.pos.reserve((size_t)V * 3, H));
    PSGPU_CHECK(W.nrm.reserve((size_t)V * 3, H));
    PSGPU_CHECK(W.col.reserve((size_t)V * 3, H));
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
    q.mapBlocks = (V + 4u * kWeldBlock - 1u) / (4u * kWeldBlock);
    *slotsOut = slots;
    return PSGPU_RET_SUCCESS;
}

// The launches after the mark, shared by psgpu_weld and a group's weld; ev (null: untimed): four
// events, one recorded after each launch.
int weld_after_mark(const WeldParams& q, hipStream_t s, hipEvent_t* ev) {
    const uint32_t triBlocks = (uint32_t)(((uint64_t)q.T + 4ull * kWeldBlock - 1ull) / (4ull * kWeldBlock));
    hipLaunchKernelGGL(k_weld_resolve, dim3(q.blocks), dim3(kWeldBlock), 0, s, q);
    if (ev) PSGPU_CHECK(hipEventRecord(ev[0], s));
    hipLaunchKernelGGL(k_weld_scan, dim3(1), dim3(kWeldBlock), 0, s, q);
    if (ev) PSGPU_CHECK(hipEventRecord(ev[1], s));
    hipLaunchKernelGGL(k_weld_emit, dim3(q.blocks), dim3(kWeldBlock), 0, s, q);
    if (ev) PSGPU_CHECK(hipEventRecord(ev[2], s));
    hipLaunchKernelGGL(k_weld_map, dim3(q.mapBlocks + triBlocks), dim3(kWeldBlock), 0, s, q);
    if (ev) PSGPU_CHECK(hipEventRecord(ev[3], s));
    PSGPU_CHECK(hipGetLastError());
    return PSGPU_RET_SUCCESS;
}

}  // namespace

// the current run is finished, uncollected by nothing newer, and whole
bool weld_run_ready(const psgpu_ctx* c) {
    return c && !c->pending && c->haveResult && c->finishedSeq == c->runSeq;
}

void weld_state_free(WeldState& W) {
    for (hipEvent_t e : W.filter.ev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : W.shells.ev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : W.ev)
        if (e) (void)hipEventDestroy(e);
    W = WeldState{};  // releases the weld's buffers, the shells' and the filter's
}

void weld_free(psgpu_ctx* c) { weld_state_free(c->weld); }

void weld_scan_blocks(uint64_t* blockCnt, uint32_t blocks, hipStream_t s) {
    WeldParams q;
    memset(&q, 0, sizeof(q));
    q.blockCnt = blockCnt;
    q.blocks = blocks;
    hipLaunchKernelGGL(k_weld_scan, dim3(1), dim3(kWeldBlock), 0, s, q);
}

int weld_edges(psgpu_ctx* c, uint64_t* edge, hipStream_t s) {
    const uint32_t V = c->info.ctVertices;
    if (V == 0) return PSGPU_RET_SUCCESS;
    WeldEdgeParams q;
    memset(&q, 0, sizeof(q));
    const int rc = weld_shard_counts(c, V, q.shardV);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    q.vk = c->vk;
    q.offs = c->offs;
    q.vShardCap = c->vShardCap;
    for (int a = 0; a < 3; ++a) q.dims[a] = c->dims[a];
    q.mpuBegin = c->mpuBegin;
    q.mpuCount = c->mpuCount;
    q.V = V;
    q.edge = edge;
    PSGPU_CHECK(hipMemsetAsync(edge, 0xff, (size_t)V * 8, s));
    hipLaunchKernelGGL(k_weld_edges, dim3((V + kWeldBlock - 1) / kWeldBlock), dim3(kWeldBlock), 0, s, q);
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
    if (pos && V) PSGPU_CHECK(hipMemcpy(pos, W.pos, V * 12, hipMemcpyDeviceToHost));
    if (nrm && V) PSGPU_CHECK(hipMemcpy(nrm, W.nrm, V * 12, hipMemcpyDeviceToHost));
    if (col && V) PSGPU_CHECK(hipMemcpy(col, W.col, V * 12, hipMemcpyDeviceToHost));
    if (tris && T) PSGPU_CHECK(hipMemcpy(tris, W.tris, T * 12, hipMemcpyDeviceToHost));
    if (vertexMap && Vin) PSGPU_CHECK(hipMemcpy(vertexMap, W.map, Vin * 4, hipMemcpyDeviceToHost));
    return PSGPU_RET_SUCCESS;
}

int weld_gathered(WeldState& W, const WeldGathered& in, hipStream_t s, hipEvent_t* ev, uint64_t* totals) {
    WeldParams q;
    memset(&q, 0, sizeof(q));
    uint32_t slots = 0;
    const int rc = weld_prepare(W, in.V, in.T, q, &slots);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    q.pos = in.pos;
    q.nrm = in.nrm;
    q.col = in.col;
    q.tris = in.tris;
    PSGPU_CHECK(hipMemsetAsync(W.table, 0xff, (size_t)slots * 12, s));
    hipLaunchKernelGGL(k_weld_mark_ids, dim3(q.blocks), dim3(kWeldBlock), 0, s, q, in.edge);
    if (ev) PSGPU_CHECK(hipEventRecord(ev[0], s));
    const int rt = weld_after_mark(q, s, ev ? ev + 1 : nullptr);
    if (rt != PSGPU_RET_SUCCESS) return rt;
    PSGPU_CHECK(hipMemcpyAsync(totals, W.blockCnt + q.blocks, sizeof(*totals), hipMemcpyDeviceToHost, s));
    return PSGPU_RET_SUCCESS;
}

}  // namespace psgpu

using namespace psgpu;

extern "C" {

int psgpu_weld(psgpu_ctx* c, PsWeldInfo* info) {
    if (!weld_run_ready(c)) return PSGPU_RET_PARAM_ERROR;
    if (c->info.firstOverflowMPU >= 0) return PSGPU_RET_PARAM_ERROR;  // past the reference's 512 per MPU (records complete)
    for (int a = 0; a < 3; ++a)
        if (7ull * c->dims[a] >= (1ull << kCoordBits)) return PSGPU_RET_PARAM_ERROR;
    int rc = set_device(c);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    WeldState& W = c->weld;
    const uint32_t V = c->info.ctVertices, T = c->info.ctTriangles;
    W.doneSeq = ~0ull;
    W.shells.valid = false;
    W.filter.valid = false;
    memset(&W.info, 0, sizeof(W.info));
    W.info.ctInputVertices = V;
    W.info.ctTriangles = T;
    for (float& ms : W.lastMs) ms = 0.0f;
    if (V == 0) {  // nothing to launch: an empty mesh welds to an empty mesh
        W.doneSeq = c->runSeq;
        if (info) *info = W.info;
        return PSGPU_RET_SUCCESS;
    }
    WeldParams q;
    memset(&q, 0, sizeof(q));
    rc = weld_shard_counts(c, V, q.shardV);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    uint32_t slots = 0;
    rc = weld_prepare(W, V, T, q, &slots);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    q.vk = c->vk;
    q.offs = c->offs;
    q.vShardCap = c->vShardCap;
    for (int a = 0; a < 3; ++a) q.dims[a] = c->dims[a];
    q.mpuBegin = c->mpuBegin;
    q.mpuCount = c->mpuCount;
    q.pos = c->pos;
    q.nrm = c->nrm;
    q.col = c->col;
    q.tris = c->tris;
    hipStream_t s = c->stream;
    const bool timed = c->timing != 0;
    if (timed)
        for (hipEvent_t& e : W.ev)
            if (!e) PSGPU_CHECK(hipEventCreate(&e));
    if (timed) PSGPU_CHECK(hipEventRecord(W.ev[0], s));
    // every key empty (all ones), every minimum 0xffffffff
    PSGPU_CHECK(hipMemsetAsync(W.table, 0xff, (size_t)slots * 12, s));
    hipLaunchKernelGGL(k_weld_mark, dim3(q.blocks), dim3(kWeldBlock), 0, s, q);
    if (timed) PSGPU_CHECK(hipEventRecord(W.ev[1], s));
    rc = weld_after_mark(q, s, timed ? W.ev + 2 : nullptr);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    uint64_t totals = 0;
    PSGPU_CHECK(hipMemcpyAsync(&totals, W.blockCnt + q.blocks, sizeof(totals), hipMemcpyDeviceToHost, s));
    PSGPU_CHECK(hipStreamSynchronize(s));
    if (timed) {
        (void)hipEventElapsedTime(&W.lastMs[0], W.ev[0], W.ev[kWeldPhases - 1]);
        for (int k = 1; k < kWeldPhases; ++k) (void)hipEventElapsedTime(&W.lastMs[k], W.ev[k - 1], W.ev[k]);
    }
    W.info.ctVertices = (uint32_t)totals;
    W.info.ctSeamVertices = (uint32_t)(totals >> 32);
    W.doneSeq = c->runSeq;
    if (info) *info = W.info;
    return PSGPU_RET_SUCCESS;
}

int psgpu_weld_device(psgpu_ctx* c, PsWeldDevice* out) {
    if (!out || !weld_run_ready(c) || c->weld.doneSeq != c->runSeq) return PSGPU_RET_PARAM_ERROR;
    return weld_device(c->weld, out);
}

int psgpu_download_weld(psgpu_ctx* c, float* pos, float* nrm, float* col, uint32_t* tris, uint32_t* vertexMap) {
    if (!weld_run_ready(c) || c->weld.doneSeq != c->runSeq) return PSGPU_RET_PARAM_ERROR;
    const int rc = set_device(c);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    return weld_download(c->weld, pos, nrm, col, tris, vertexMap);
}

int psgpu_weld_times(psgpu_ctx* c, float* ms, int maxPhases, const char** names) {
    if (!c) return 0;
    const int n = std::min(maxPhases, kWeldPhases);
    for (int k = 0; k < n; ++k) {
        if (ms) ms[k] = c->weld.lastMs[k];
        if (names) names[k] = kWeldPhaseNames[k];
    }
    return n;
}

}  // extern "C"
