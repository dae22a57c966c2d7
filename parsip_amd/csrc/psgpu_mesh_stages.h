// psgpu_mesh_stages.h — the device stages that the kernels of psgpu_weld.hip, psgpu_shells.hip
// and psgpu_filter.hip are built from (DESIGN.md §6 "Mesh stages").  Every kernel of the three
// runs blocks of kMeshBlock lanes, one element (vertex, triangle, shell, record) a lane.
//
//   mesh_hash, table_claim  the open-addressing tables: k_weld_mark, k_weld_mark_ids (edge id ->
//                           smallest vertex), k_shells_edges (edge -> uses)
//   record_edge_id          a vertex record as its lattice edge: k_weld_mark, k_weld_edges
//   block_rank              a lane's place among the block's flagged lanes, and their number:
//                           every kernel that counts or compacts
//   stage_in, stage_out,    the stable compaction of three-word elements through LDS:
//   compact3                k_weld_emit, k_filter_emit; k_filter_tris maps between the two stages
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "psgpu_model.h"

namespace psgpu {

constexpr uint32_t kMeshBlock = 256;
constexpr uint32_t kMeshWaves = kMeshBlock / 64;
constexpr uint32_t kNoSlot = 0xffffffffu;
constexpr uint64_t kEmptyKey = ~0ull;  // a free table slot: the weld's edge ids use 62 bits, the shells' edges have lo < hi
constexpr uint32_t kCoordBits = 20;    // per lattice coordinate of an edge id (weld_lattice_fits)

inline uint32_t mesh_blocks(uint64_t n) { return (uint32_t)((n + kMeshBlock - 1) / kMeshBlock); }

__device__ __forceinline__ uint32_t mesh_hash(uint64_t x) {  // murmur3's 64-bit finaliser
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return (uint32_t)x;
}

// The slot of `key` in a table of mask + 1 keys, claimed if no lane had yet.  The hosts size
// their tables so that at most half the slots are ever taken: an empty or matching slot comes
// up, and the bound only keeps a corrupt input from spinning (kNoSlot then).
__device__ __forceinline__ uint32_t table_claim(uint64_t* keys, uint32_t mask, uint64_t key) {
    uint32_t slot = mesh_hash(key) & mask;
    for (uint32_t tries = 0; tries <= mask; ++tries) {
        const uint64_t seen = atomicCAS((unsigned long long*)&keys[slot], (unsigned long long)kEmptyKey,
                                        (unsigned long long)key);
        if (seen == kEmptyKey || seen == key) return slot;
        slot = (slot + 1u) & mask;
    }
    return kNoSlot;
}

// A finished run's vertex records: record (w, vid, key) of shard k is mesh vertex
// offs[w] + vid on the lattice edge that `key` names inside MPU w + mpuBegin.
struct WeldRecords {
    const VertexKey* vk;
    const uint64_t* offs;
    uint32_t vShardCap;
    uint32_t shardV[kShards];  // vertex records per shard (the run's host counters)
    uint32_t dims[3];
    uint32_t mpuBegin, mpuCount;
};

// Record blockIdx.x * kMeshBlock + threadIdx.x of a run of V vertices: *gi its mesh vertex
// (kNoSlot: there is no such record) and, for a vertex on an MPU face (an off-axis coordinate
// on the MPU's first or last corner plane), the id of its global lattice edge
//     (7 i + sx, 7 j + sy, 7 k + sz, axis),  (i, j, k) = MPU w + mpuBegin in x-major order;
// kEmptyKey for every other.  Every lane of the block calls this (one barrier: sStart).
__device__ __forceinline__ uint64_t record_edge_id(const WeldRecords& q, uint32_t V, uint32_t* sStart, uint32_t* gi) {
    if (threadIdx.x == 0) {
        uint32_t at = 0;
        for (int k = 0; k < kShards; ++k) {
            sStart[k] = at;
            at += q.shardV[k];
        }
        sStart[kShards] = at;
    }
    __syncthreads();
    *gi = kNoSlot;
    const uint32_t r = blockIdx.x * kMeshBlock + threadIdx.x;
    if (r >= sStart[kShards]) return kEmptyKey;
    uint32_t shard = 0;  // the last shard whose first record is <= r
    for (uint32_t step = kShards / 2; step; step >>= 1)
        if (sStart[shard + step] <= r) shard += step;
    const VertexKey K = q.vk[(size_t)shard * q.vShardCap + (r - sStart[shard])];
    if (K.w >= q.mpuCount) return kEmptyKey;
    const uint32_t v = (uint32_t)q.offs[K.w] + (K.vidKey & 0xffffu);
    if (v >= V) return kEmptyKey;
    *gi = v;
    const uint32_t key = K.vidKey >> 16;
    const uint32_t sx = key & 7u, sy = (key >> 3) & 7u, sz = (key >> 6) & 7u, ax = (key >> 9) & 3u;
    const bool fx = sx == 0u || sx == 7u, fy = sy == 0u || sy == 7u, fz = sz == 0u || sz == 7u;
    if (!((ax != 0u && fx) || (ax != 1u && fy) || (ax != 2u && fz))) return kEmptyKey;
    const uint32_t m = K.w + q.mpuBegin;
    const uint32_t nyz = q.dims[1] * q.dims[2];
    const uint32_t i = m / nyz, jk = m - i * nyz;
    const uint32_t j = jk / q.dims[2], k = jk - j * q.dims[2];
    return ((((uint64_t)(7u * i + sx) << kCoordBits | (uint64_t)(7u * j + sy)) << kCoordBits | (uint64_t)(7u * k + sz))
            << 2) | ax;
}

// block_rank in two halves, for a kernel that ranks two flags across one barrier
// (k_weld_resolve): wave_rank posts the wave's count to sWave[wave] and returns the lane's
// place in its wave; after a __syncthreads(), block_rank_sum adds the waves below.
__device__ __forceinline__ uint32_t wave_rank(bool flag, uint32_t* sWave) {
    const uint64_t b = __ballot(flag);
    const uint32_t lane = threadIdx.x & 63u;
    if (lane == 0u) sWave[threadIdx.x >> 6] = (uint32_t)__popcll(b);
    return (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
}
__device__ __forceinline__ uint32_t block_rank_sum(uint32_t at, const uint32_t* sWave, uint32_t* total) {
    uint32_t n = 0;
    for (uint32_t w = 0; w < kMeshWaves; ++w) {
        if (w < (threadIdx.x >> 6)) at += sWave[w];
        n += sWave[w];
    }
    *total = n;
    return at;
}

// This lane's place among the block's lanes with the flag set; *total: how many have it.
// Every lane of the block calls this (one barrier).  sWave: kMeshWaves words that no lane
// still reads: a kernel that calls twice with one array puts a barrier between.
__device__ __forceinline__ uint32_t block_rank(bool flag, uint32_t* sWave, uint32_t* total) {
    const uint32_t at = wave_rank(flag, sWave);
    __syncthreads();
    return block_rank_sum(at, sWave, total);
}

// Three words an element (a vertex attribute, a triangle's corners) of the block's elements
// [i0, i0 + n): 16-byte loads into LDS.  i0 is a multiple of kMeshBlock, so src + 3 i0 is
// 16-byte aligned, as sIn must be.
__device__ __forceinline__ void stage_in(const uint32_t* __restrict__ src, uint32_t i0, uint32_t n, uint32_t* sIn) {
    const uint32_t words = 3u * n;
    const uint32_t* s = src + (size_t)i0 * 3u;
    for (uint32_t x = threadIdx.x * 4u; x < words; x += kMeshBlock * 4u) {
        if (x + 4u <= words) {
            *reinterpret_cast<uint4*>(sIn + x) = *reinterpret_cast<const uint4*>(s + x);
        } else {
            for (uint32_t y = x; y < words; ++y) sIn[y] = s[y];
        }
    }
    __syncthreads();
}

// the block's nKept compacted elements in sOut as consecutive words from element `base` of
// dst; sIn and sOut are free again when it returns
__device__ __forceinline__ void stage_out(uint32_t* __restrict__ dst, uint32_t base, uint32_t nKept, const uint32_t* sOut) {
    __syncthreads();
    uint32_t* d = dst + (size_t)base * 3u;
    for (uint32_t x = threadIdx.x; x < 3u * nKept; x += kMeshBlock) d[x] = sOut[x];
    __syncthreads();
}

// One attribute array: the kept ones of the block's vertices [i0, i0 + n) of src, in order and
// bit for bit, as vertices [base, base + nKept) of dst; this lane's vertex is the at-th kept
// one (block_rank).
__device__ __forceinline__ void compact3(const float* src, float* dst, uint32_t i0, uint32_t n, bool kept, uint32_t at,
                                         uint32_t nKept, uint32_t base, uint32_t* sIn, uint32_t* sOut) {
    stage_in(reinterpret_cast<const uint32_t*>(src), i0, n, sIn);
    if (kept)
        for (uint32_t k = 0; k < 3u; ++k) sOut[3u * at + k] = sIn[3u * threadIdx.x + k];
    stage_out(reinterpret_cast<uint32_t*>(dst), base, nKept, sOut);
}

}  // namespace psgpu
