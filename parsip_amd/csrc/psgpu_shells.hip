// psgpu_shells.hip — the shells of a welded mesh: connected components with their topology,
// area and volume (psgpu_weld_shells / psgpu_group_weld_shells, include/parsip_gpu.h, whose
// "Reproducible measures" rule the kernels below follow term for term).
//
// The input is a WeldState's welded arrays (pos, tris), a context's or a group's alike.
//
//   k_shells_init       one lane per vertex: parent[v] = v; the largest |coordinate|
//   k_shells_edges      one lane per triangle: its three edges {lo < hi} enter an
//                       open-addressing table (table_claim of lo << 32 | hi), then a 64-bit
//                       atomic add counts the use (lo->hi: low word, hi->lo: high word)
//   k_shells_union      one lane per triangle: lock-free union-find, the larger root hooked
//                       under the smaller by CAS, so a component's root is its smallest vertex
//   k_shells_flatten    one lane per vertex: its root; roots per block (block_rank)
//   k_weld_scan         (psgpu_weld.hip) the block counts scanned; the host reads the shell
//                       count, the error word and the largest coordinate, sizes the per-shell
//                       buffers and fixes the scales eA, eV
//   k_shells_ids        one lane per vertex: a root's shell index (block_rank + base), its
//                       accumulator cleared
//   k_shells_vertices   one lane per vertex: vertexShell; count and bounding box
//   k_shells_edge_class one lane per table slot: the edge's class into its shell
//   k_shells_triangles  one lane per triangle: triShell; count and the four integers
//   k_shells_finish     one lane per shell: its PsShell; the mesh totals
//
// table_claim and block_rank are psgpu_mesh_stages.h's, shared with the weld and the filter.
//
// The phases are ordered by kernel boundaries alone: no block waits for another inside a
// launch.  Every loop is bounded; a bound that is hit sets the error word and the call returns
// PSGPU_RET_DEVICE_ERROR.  Every value written is a function of the welded arrays: slots and
// the shape of the union-find forest depend on arrival order, roots, counts, minima, maxima
// and integer sums do not.
//
// The three accumulate kernels add into one record per shell.  A mesh that is one shell would
// put every atomic on one address, so lanes that agree on the shell reduce first: a wave
// reduces the lanes of each distinct shell among its own by shuffles, adds once per shell to
// the block's records in LDS (eight shells at most; any further one goes to HBM directly), and
// the block adds its records to HBM once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "psgpu_internal.h"
#include "psgpu_mesh_stages.h"

namespace psgpu {

namespace {

enum : uint32_t { kErrIndex = 1u, kErrTable = 2u, kErrUnion = 4u };  // ShellsCtl::err

// counts, bounding box keys (float_key: unsigned order = float order) and the integer sums of
// one shell; the mesh totals are one more of these
enum : int { cFirst, cV, cT, cE, cOpen, cNonManifold, cFlipped, cClosed };  // ShellAcc::cnt
struct ShellAcc {
    uint32_t cnt[8];  // the first vertex, then counts: vertices, triangles, edges and their classes, closed shells
    uint32_t lo[3], hi[3];
    unsigned long long sum[4];  // A2 hi, A2 lo, V6 hi, V6 lo (two's complement)
};
struct ShellsCtl {
    uint32_t err;
    uint32_t maxBits;  // bits of the largest |coordinate|
    ShellAcc total;
};

struct ShellsParams {
    const float* pos;
    const uint32_t* tris;
    uint32_t V, T;
    uint64_t* keys;            // table: tableMask + 1 edges ...
    unsigned long long* uses;  // ... and their uses, f | b << 32
    uint32_t tableMask;
    uint32_t* parent;
    uint32_t* vertexShell;
    uint32_t* triShell;
    uint64_t* blockCnt;
    ShellsCtl* ctl;
    ShellAcc* acc;
    PsShell* shells;
    uint32_t S;
    int eA, eV;
};

__device__ __forceinline__ uint32_t float_key(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_float(uint32_t k) {
    return __uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k);
}

__global__ void __launch_bounds__(kMeshBlock) k_shells_init(ShellsParams q) {
    __shared__ uint32_t sMax[kMeshWaves];
    const uint32_t v = blockIdx.x * kMeshBlock + threadIdx.x;
    uint32_t m = 0;
    if (v < q.V) {
        q.parent[v] = v;
        const float* p = q.pos + (size_t)v * 3u;
        // |x| of a finite float: its bits order as its value
        m = max(max(__float_as_uint(fabsf(p[0])), __float_as_uint(fabsf(p[1]))), __float_as_uint(fabsf(p[2])));
    }
    for (uint32_t d = 32; d; d >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, (int)d, 64));
    if ((threadIdx.x & 63u) == 0u) sMax[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < kMeshWaves; ++w) m = max(m, sMax[w]);
        if (m) atomicMax(&q.ctl->maxBits, m);
    }
}

// one use of edge x -> y
__device__ __forceinline__ void edge_use(const ShellsParams& q, uint32_t x, uint32_t y) {
    if (x == y) return;
    const uint32_t slot = table_claim(q.keys, q.tableMask, (uint64_t)min(x, y) << 32 | max(x, y));
    if (slot != kNoSlot)
        atomicAdd(&q.uses[slot], x < y ? 1ull : 1ull << 32);
    else
        atomicOr(&q.ctl->err, kErrTable);
}

__global__ void __launch_bounds__(kMeshBlock) k_shells_edges(ShellsParams q) {
    const uint32_t t = blockIdx.x * kMeshBlock + threadIdx.x;
    if (t >= q.T) return;
    const uint32_t* c = q.tris + (size_t)t * 3u;
    const uint32_t a = c[0], b = c[1], d = c[2];
    if (a >= q.V || b >= q.V || d >= q.V) {
        atomicOr(&q.ctl->err, kErrIndex);
        return;
    }
    edge_use(q, a, b);
    edge_use(q, b, d);
    edge_use(q, d, a);
}

__device__ __forceinline__ uint32_t parent_of(const uint32_t* parent, uint32_t x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root above x.  parent[x] <= x always, with equality at a root only, so the walk descends
// and ends within x steps; on the way every vertex passed is moved under its grandparent
// (atomicMin: a parent only ever becomes a smaller ancestor).
__device__ __forceinline__ uint32_t shell_find(uint32_t* parent, uint32_t x) {
    uint32_t p = parent_of(parent, x);
    while (p < x) {
        const uint32_t gp = parent_of(parent, p);
        if (gp < p) atomicMin(parent + x, gp);
        x = p;
        p = gp;
    }
    return x;
}

// Joins the sets of x and y: the larger root goes under the smaller.  A failed CAS means
// another lane hooked that root meanwhile; there are fewer than V hooks in all, so V tries
// are never used up.
__device__ __forceinline__ void shell_union(const ShellsParams& q, uint32_t x, uint32_t y) {
    for (uint32_t tries = 0; tries <= q.V; ++tries) {
        x = shell_find(q.parent, x);
        y = shell_find(q.parent, y);
        if (x == y) return;
        const uint32_t hi = max(x, y), lo = min(x, y);
        if (atomicCAS(q.parent + hi, hi, lo) == hi) return;
    }
    atomicOr(&q.ctl->err, kErrUnion);
}

__global__ void __launch_bounds__(kMeshBlock) k_shells_union(ShellsParams q) {
    const uint32_t t = blockIdx.x * kMeshBlock + threadIdx.x;
    if (t >= q.T) return;
    const uint32_t* c = q.tris + (size_t)t * 3u;
    const uint32_t a = c[0], b = c[1], d = c[2];
    if (a >= q.V || b >= q.V || d >= q.V) return;  // k_shells_edges has set the error
    shell_union(q, a, b);
    shell_union(q, b, d);
}

__global__ void __launch_bounds__(kMeshBlock) k_shells_flatten(ShellsParams q) {
    __shared__ uint32_t sRoots[kMeshWaves];
    const uint32_t v = blockIdx.x * kMeshBlock + threadIdx.x;
    bool root = false;
    if (v < q.V) {
        const uint32_t r = shell_find(q.parent, v);
        q.vertexShell[v] = r;
        root = r == v;
    }
    uint32_t n;
    (void)block_rank(root, sRoots, &n);
    if (threadIdx.x == 0) q.blockCnt[blockIdx.x] = n;
}

__device__ __forceinline__ void acc_clear(ShellAcc* a, uint32_t first) {
    for (int i = 0; i < 8; ++i) a->cnt[i] = 0u;
    a->cnt[cFirst] = first;
    for (int i = 0; i < 3; ++i) {
        a->lo[i] = 0xffffffffu;
        a->hi[i] = 0u;
    }
    for (int i = 0; i < 4; ++i) a->sum[i] = 0ull;
}

// a root's shell index, left in parent[root]; vertexShell still holds every vertex's root
__global__ void __launch_bounds__(kMeshBlock) k_shells_ids(ShellsParams q) {
    __shared__ uint32_t sWave[kMeshWaves];
    const uint32_t v = blockIdx.x * kMeshBlock + threadIdx.x;
    const bool root = v < q.V && q.vertexShell[v] == v;
    uint32_t roots;
    const uint32_t at = block_rank(root, sWave, &roots);
    if (root) {
        const uint32_t s = (uint32_t)q.blockCnt[blockIdx.x] + at;
        if (s < q.S) {
            q.parent[v] = s;
            acc_clear(q.acc + s, v);
        }
    }
    if (v == 0u) acc_clear(&q.ctl->total, 0u);
}

// ---- accumulation into the shells' records ---------------------------------------------------

enum Kind { kVertices, kEdges, kTriangles, kTotals };

// which fields of a ShellAcc a kind of part carries: bit i for cnt[i], the box, the sums
constexpr uint32_t kind_counts(Kind k) {
    return k == kVertices    ? 1u << cV
           : k == kEdges     ? 1u << cE | 1u << cOpen | 1u << cNonManifold | 1u << cFlipped
           : k == kTriangles ? 1u << cT
                             : 0xfeu;
}
constexpr bool kind_box(Kind k) { return k == kVertices || k == kTotals; }
constexpr bool kind_sums(Kind k) { return k == kTriangles || k == kTotals; }

__device__ __forceinline__ ShellAcc part_none() {
    ShellAcc p;
    acc_clear(&p, 0u);
    return p;
}

template <Kind K>
__device__ __forceinline__ void part_merge(ShellAcc& p, const ShellAcc& o) {
    for (int i = 0; i < 8; ++i)
        if (kind_counts(K) >> i & 1u) p.cnt[i] += o.cnt[i];
    if (kind_box(K))
        for (int i = 0; i < 3; ++i) {
            p.lo[i] = min(p.lo[i], o.lo[i]);
            p.hi[i] = max(p.hi[i], o.hi[i]);
        }
    if (kind_sums(K))
        for (int i = 0; i < 4; ++i) p.sum[i] += o.sum[i];
}

template <Kind K>
__device__ __forceinline__ ShellAcc part_shfl_xor(const ShellAcc& p, int d) {
    ShellAcc o = p;
    for (int i = 0; i < 8; ++i)
        if (kind_counts(K) >> i & 1u) o.cnt[i] = (uint32_t)__shfl_xor((int)p.cnt[i], d, 64);
    if (kind_box(K))
        for (int i = 0; i < 3; ++i) {
            o.lo[i] = (uint32_t)__shfl_xor((int)p.lo[i], d, 64);
            o.hi[i] = (uint32_t)__shfl_xor((int)p.hi[i], d, 64);
        }
    if (kind_sums(K))
        for (int i = 0; i < 4; ++i) o.sum[i] = (unsigned long long)__shfl_xor((long long)p.sum[i], d, 64);
    return o;
}

// a += p, by atomics (a in HBM or in LDS); zero counts of the rare edge classes are skipped
template <Kind K>
__device__ __forceinline__ void part_add(ShellAcc* a, const ShellAcc& p) {
    for (int i = 0; i < 8; ++i)
        if ((kind_counts(K) >> i & 1u) && p.cnt[i]) atomicAdd(&a->cnt[i], p.cnt[i]);
    if (kind_box(K))
        for (int i = 0; i < 3; ++i) {
            atomicMin(&a->lo[i], p.lo[i]);
            atomicMax(&a->hi[i], p.hi[i]);
        }
    if (kind_sums(K))
        for (int i = 0; i < 4; ++i) atomicAdd(&a->sum[i], p.sum[i]);
}

// the sum of the parts of the lanes with `in` set (every lane of the wave calls this), in all of them
template <Kind K>
__device__ __forceinline__ ShellAcc wave_sum(const ShellAcc& mine, bool in) {
    ShellAcc r = in ? mine : part_none();
    if (K == kEdges) {  // flags: counted by ballots
        for (int i = cE; i <= cFlipped; ++i) r.cnt[i] = (uint32_t)__popcll(__ballot(in && mine.cnt[i] != 0u));
        return r;
    }
    for (int d = 32; d; d >>= 1) {
        const ShellAcc o = part_shfl_xor<K>(r, d);
        part_merge<K>(r, o);
    }
    return r;
}

// A block's sums in LDS: the first kHeld shells its waves name each get a record here, which
// goes to HBM once when the block ends; a shell that finds no record goes to HBM directly.
constexpr uint32_t kHeld = 8;
constexpr uint32_t kNoShell = 0xffffffffu;
struct BlockSums {
    uint32_t shell[kHeld];
    ShellAcc acc[kHeld];
};

__device__ __forceinline__ void block_begin(BlockSums& sh) {
    if (threadIdx.x < kHeld) {
        sh.shell[threadIdx.x] = kNoShell;
        acc_clear(&sh.acc[threadIdx.x], 0u);
    }
    __syncthreads();
}

// Adds the active lanes' parts to their shells (s < the number of shells).  Every lane of the
// wave calls this, active or not, between block_begin and block_end.  The wave adds one
// reduced part per distinct shell among its lanes (a lane alone with its shell adds its own).
// Sums, minima and maxima are order-free, so the route a part takes changes no bit.
template <Kind K>
__device__ __forceinline__ void wave_add(ShellAcc* acc, uint32_t s, bool active, const ShellAcc& mine, BlockSums& sh) {
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t rest = __ballot(active);
    while (rest) {  // wave-uniform; every pass takes the first remaining lane's shell out, 64 passes at most
        const uint32_t leader = (uint32_t)__ffsll((unsigned long long)rest) - 1u;
        const uint32_t sl = (uint32_t)__shfl((int)s, (int)leader, 64);
        const bool in = active && s == sl;
        const uint64_t group = __ballot(in);
        ShellAcc g = mine;
        if (__popcll(group) > 1) g = wave_sum<K>(mine, in);
        if (lane == leader) {
            bool held = false;
            for (uint32_t i = 0; i < kHeld && !held; ++i) {
                const uint32_t seen = atomicCAS(&sh.shell[i], kNoShell, sl);
                if (seen == kNoShell || seen == sl) {
                    part_add<K>(&sh.acc[i], g);
                    held = true;
                }
            }
            if (!held) part_add<K>(acc + sl, g);
        }
        rest &= ~group;
    }
}

template <Kind K>
__device__ __forceinline__ void block_end(ShellAcc* acc, BlockSums& sh) {
    __syncthreads();
    if (threadIdx.x < kHeld && sh.shell[threadIdx.x] != kNoShell)
        part_add<K>(acc + sh.shell[threadIdx.x], sh.acc[threadIdx.x]);
}

__global__ void __launch_bounds__(kMeshBlock) k_shells_vertices(ShellsParams q) {
    __shared__ BlockSums sh;
    block_begin(sh);
    const uint32_t v = blockIdx.x * kMeshBlock + threadIdx.x;
    bool active = v < q.V;
    uint32_t s = 0;
    ShellAcc p = part_none();
    if (active) {
        s = q.parent[q.vertexShell[v]];  // the root's shell index
        active = s < q.S;
        if (active) {
            q.vertexShell[v] = s;
            const float* x = q.pos + (size_t)v * 3u;
            p.cnt[cV] = 1u;
            for (int i = 0; i < 3; ++i) p.lo[i] = p.hi[i] = float_key(x[i]);
        }
    }
    wave_add<kVertices>(q.acc, s, active, p, sh);
    block_end<kVertices>(q.acc, sh);
}

constexpr uint32_t kSlotsPerLane = 8;  // k_shells_edge_class: most slots are empty

__global__ void __launch_bounds__(kMeshBlock) k_shells_edge_class(ShellsParams q) {
    __shared__ BlockSums sh;
    block_begin(sh);
    for (uint32_t it = 0; it < kSlotsPerLane; ++it) {
        const uint64_t slot = ((uint64_t)blockIdx.x * kSlotsPerLane + it) * kMeshBlock + threadIdx.x;
        bool active = false;
        uint32_t s = 0;
        ShellAcc p = part_none();
        if (slot <= q.tableMask) {
            const uint64_t key = q.keys[slot];
            if (key != kEmptyKey) {
                const uint32_t lo = (uint32_t)(key >> 32);
                if (lo < q.V) s = q.vertexShell[lo];
                active = lo < q.V && s < q.S;
                const unsigned long long u = q.uses[slot];
                const uint64_t f = u & 0xffffffffull, b = u >> 32, n = f + b;
                p.cnt[cE] = 1u;
                p.cnt[cOpen] = n == 1u;
                p.cnt[cNonManifold] = n >= 3u;
                p.cnt[cFlipped] = n == 2u && f != b;
            }
        }
        wave_add<kEdges>(q.acc, s, active, p, sh);
    }
    block_end<kEdges>(q.acc, sh);
}

// x at scale e as two integers (parsip_gpu.h, step 3)
__device__ __forceinline__ void term_split(double x, int e, unsigned long long* hi, unsigned long long* lo) {
    const double y = ldexp(x, e);
    const double h = floor(y);
    *hi = (unsigned long long)(long long)h;
    *lo = (unsigned long long)(long long)floor((y - h) * 1073741824.0);
}

__global__ void __launch_bounds__(kMeshBlock) k_shells_triangles(ShellsParams q) {
    __shared__ BlockSums sh;
    block_begin(sh);
    const uint32_t t = blockIdx.x * kMeshBlock + threadIdx.x;
    bool active = false;
    uint32_t s = 0;
    ShellAcc p = part_none();
    if (t < q.T) {
        const uint32_t* c = q.tris + (size_t)t * 3u;
        const uint32_t ia = c[0], ib = c[1], ic = c[2];
        if (ia < q.V && ib < q.V && ic < q.V) {
            s = q.vertexShell[ia];
            active = s < q.S;
        }
        if (active) {
            q.triShell[t] = s;
            const float *pa = q.pos + (size_t)ia * 3u, *pb = q.pos + (size_t)ib * 3u, *pc = q.pos + (size_t)ic * 3u;
            const double ax = pa[0], ay = pa[1], az = pa[2];
            const double bx = pb[0], by = pb[1], bz = pb[2];
            const double cx = pc[0], cy = pc[1], cz = pc[2];
            const double ux = bx - ax, uy = by - ay, uz = bz - az;
            const double vx = cx - ax, vy = cy - ay, vz = cz - az;
            const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
            const double a2 = sqrt(nx * nx + ny * ny + nz * nz);
            const double v6 = ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz) + az * (bx * cy - by * cx);
            p.cnt[cT] = 1u;
            term_split(a2, q.eA, &p.sum[0], &p.sum[1]);
            term_split(v6, q.eV, &p.sum[2], &p.sum[3]);
        }
    }
    wave_add<kTriangles>(q.acc, s, active, p, sh);
    block_end<kTriangles>(q.acc, sh);
}

// two accumulators as a value (parsip_gpu.h, step 5); the same expression on the host for the totals
__host__ __device__ inline double sums_value(unsigned long long hi, unsigned long long lo, int e, double div) {
    return (ldexp((double)(long long)hi, -e) + ldexp((double)(long long)lo, -e - 30)) / div;
}

__global__ void __launch_bounds__(kMeshBlock) k_shells_finish(ShellsParams q) {
    __shared__ BlockSums sh;
    block_begin(sh);
    const uint32_t s = blockIdx.x * kMeshBlock + threadIdx.x;
    const bool active = s < q.S;
    ShellAcc a = part_none();
    if (active) {
        a = q.acc[s];
        PsShell o;
        o.firstVertex = a.cnt[cFirst];
        o.ctVertices = a.cnt[cV];
        o.ctTriangles = a.cnt[cT];
        o.ctEdges = a.cnt[cE];
        o.ctOpenEdges = a.cnt[cOpen];
        o.ctNonManifoldEdges = a.cnt[cNonManifold];
        o.ctFlippedEdges = a.cnt[cFlipped];
        o.euler = (int32_t)(a.cnt[cV] - a.cnt[cE] + a.cnt[cT]);
        o.area = sums_value(a.sum[0], a.sum[1], q.eA, 2.0);
        o.volume = sums_value(a.sum[2], a.sum[3], q.eV, 6.0);
        for (int i = 0; i < 3; ++i) {
            o.bboxLo[i] = key_float(a.lo[i]);
            o.bboxHi[i] = key_float(a.hi[i]);
        }
        q.shells[s] = o;
        a.cnt[cClosed] = a.cnt[cT] > 0u && !a.cnt[cOpen] && !a.cnt[cNonManifold] && !a.cnt[cFlipped];
    }
    // every shell's record adds to the one record of the totals
    wave_add<kTotals>(&q.ctl->total, 0u, active, a, sh);
    block_end<kTotals>(&q.ctl->total, sh);
}

const char* kShellsPhaseNames[kShellsPhases] = {
    "shells total",  "table fill + k_shells_init", "k_shells_edges",      "k_shells_union",     "k_shells_flatten",
    "k_weld_scan",   "k_shells_ids",               "k_shells_vertices",   "k_shells_edge_class", "k_shells_triangles",
    "k_shells_finish"};

}  // namespace

int shells_run(WeldState& W, hipStream_t s, bool timed, PsShellsInfo* info) {
    ShellsState& S = W.shells;
    const uint32_t V = W.info.ctVertices, T = W.info.ctTriangles;
    S.valid = false;
    W.filter.valid = false;
    memset(&S.info, 0, sizeof(S.info));
    S.times.clear();
    if (V == 0) {  // an empty weld: no shell, nothing to launch
        S.valid = true;
        if (info) *info = S.info;
        return PSGPU_RET_SUCCESS;
    }
    // at most 3 T edges: a table of >= 6 T slots stays at most half full
    uint64_t slots = 1024;
    while (slots < 6ull * T) slots <<= 1;
    if (slots > (1ull << 31)) return PSGPU_RET_PARAM_ERROR;
    const uint32_t blocks = mesh_blocks(V);
    constexpr Growth H = Growth::ByHalf;
    PSGPU_CHECK(S.table.reserve((size_t)slots * 16, H));
    PSGPU_CHECK(S.vertexShell.reserve((size_t)V, H));
    PSGPU_CHECK(S.parent.reserve((size_t)V, H));
    PSGPU_CHECK(S.triShell.reserve((size_t)T, H));
    PSGPU_CHECK(S.blockCnt.reserve((size_t)blocks + 1, H));
    PSGPU_CHECK(S.ctl.reserve(sizeof(ShellsCtl), H));
    ShellsParams q;
    memset(&q, 0, sizeof(q));
    q.pos = W.pos;
    q.tris = W.tris;
    q.V = V;
    q.T = T;
    q.keys = reinterpret_cast<uint64_t*>(S.table.ptr);
    q.uses = reinterpret_cast<unsigned long long*>(S.table + (size_t)slots * 8);
    q.tableMask = (uint32_t)(slots - 1);
    q.parent = S.parent;
    q.vertexShell = S.vertexShell;
    q.triShell = S.triShell;
    q.blockCnt = S.blockCnt;
    q.ctl = reinterpret_cast<ShellsCtl*>(S.ctl.ptr);
    PSGPU_CHECK(S.times.begin(timed));
    auto mark = [&]() { return S.times.mark(s); };
    const dim3 blk(kMeshBlock);
    PSGPU_CHECK(mark());
    // every key empty (all ones), every use count 0; no error, no coordinate seen
    PSGPU_CHECK(hipMemsetAsync(q.keys, 0xff, (size_t)slots * 8, s));
    PSGPU_CHECK(hipMemsetAsync(q.uses, 0, (size_t)slots * 8, s));
    PSGPU_CHECK(hipMemsetAsync(S.ctl, 0, sizeof(ShellsCtl), s));
    hipLaunchKernelGGL(k_shells_init, dim3(blocks), blk, 0, s, q);
    PSGPU_CHECK(mark());
    if (T) hipLaunchKernelGGL(k_shells_edges, dim3(mesh_blocks(T)), blk, 0, s, q);
    PSGPU_CHECK(mark());
    if (T) hipLaunchKernelGGL(k_shells_union, dim3(mesh_blocks(T)), blk, 0, s, q);
    PSGPU_CHECK(mark());
    hipLaunchKernelGGL(k_shells_flatten, dim3(blocks), blk, 0, s, q);
    PSGPU_CHECK(mark());
    weld_scan_blocks(S.blockCnt, blocks, s);
    PSGPU_CHECK(mark());
    PSGPU_CHECK(hipGetLastError());
    uint64_t roots = 0;
    uint32_t head[2] = {0, 0};  // ShellsCtl::err, maxBits
    PSGPU_CHECK(hipMemcpyAsync(&roots, S.blockCnt + blocks, sizeof(roots), hipMemcpyDeviceToHost, s));
    PSGPU_CHECK(hipMemcpyAsync(head, S.ctl, sizeof(head), hipMemcpyDeviceToHost, s));
    PSGPU_CHECK(hipStreamSynchronize(s));
    if (head[0] || roots == 0 || roots > V) return PSGPU_RET_DEVICE_ERROR;
    const uint32_t ctShells = (uint32_t)roots;
    // the scales (parsip_gpu.h, step 2): M = m 2^k with 0.5 <= m < 1, so k is the smallest with M < 2^k
    float big;
    memcpy(&big, &head[1], sizeof(big));
    int k = 0, L = 1;
    if (big > 0.0f) (void)frexpf(big, &k);
    while ((1ull << L) < (uint64_t)T) ++L;
    q.eA = 58 - 2 * k - L;
    q.eV = 58 - 3 * k - L;
    q.S = ctShells;
    PSGPU_CHECK(S.acc.reserve((size_t)ctShells * sizeof(ShellAcc), H));
    PSGPU_CHECK(S.shells.reserve((size_t)ctShells, H));
    q.acc = reinterpret_cast<ShellAcc*>(S.acc.ptr);
    q.shells = S.shells;
    hipLaunchKernelGGL(k_shells_ids, dim3(blocks), blk, 0, s, q);
    PSGPU_CHECK(mark());
    hipLaunchKernelGGL(k_shells_vertices, dim3(blocks), blk, 0, s, q);
    PSGPU_CHECK(mark());
    hipLaunchKernelGGL(k_shells_edge_class, dim3(mesh_blocks((slots + kSlotsPerLane - 1) / kSlotsPerLane)), blk, 0, s, q);
    PSGPU_CHECK(mark());
    if (T) hipLaunchKernelGGL(k_shells_triangles, dim3(mesh_blocks(T)), blk, 0, s, q);
    PSGPU_CHECK(mark());
    hipLaunchKernelGGL(k_shells_finish, dim3(mesh_blocks(ctShells)), blk, 0, s, q);
    PSGPU_CHECK(mark());
    PSGPU_CHECK(hipGetLastError());
    ShellsCtl ctl;
    PSGPU_CHECK(hipMemcpyAsync(&ctl, S.ctl, sizeof(ctl), hipMemcpyDeviceToHost, s));
    PSGPU_CHECK(hipStreamSynchronize(s));
    if (ctl.err) return PSGPU_RET_DEVICE_ERROR;
    S.times.collect();
    const ShellAcc& a = ctl.total;
    PsShellsInfo& o = S.info;
    o.ctShells = ctShells;
    o.ctClosedShells = a.cnt[cClosed];
    o.ctVertices = a.cnt[cV];
    o.ctTriangles = a.cnt[cT];
    o.ctEdges = a.cnt[cE];
    o.ctOpenEdges = a.cnt[cOpen];
    o.ctNonManifoldEdges = a.cnt[cNonManifold];
    o.ctFlippedEdges = a.cnt[cFlipped];
    o.euler = (int32_t)(a.cnt[cV] - a.cnt[cE] + a.cnt[cT]);
    o.area = sums_value(a.sum[0], a.sum[1], q.eA, 2.0);
    o.volume = sums_value(a.sum[2], a.sum[3], q.eV, 6.0);
    for (int i = 0; i < 3; ++i) {
        const uint32_t lo = a.lo[i], hi = a.hi[i];
        const uint32_t lb = (lo >> 31) ? (lo & 0x7fffffffu) : ~lo, hb = (hi >> 31) ? (hi & 0x7fffffffu) : ~hi;
        memcpy(&o.bboxLo[i], &lb, 4);
        memcpy(&o.bboxHi[i], &hb, 4);
    }
    S.valid = true;
    if (info) *info = o;
    return PSGPU_RET_SUCCESS;
}

int shells_device(const WeldState& W, PsShellsDevice* out) {
    if (!out || !W.shells.valid) return PSGPU_RET_PARAM_ERROR;
    const bool any = W.shells.info.ctShells != 0;  // an empty weld has no arrays
    out->shells = any ? W.shells.shells.ptr : nullptr;
    out->vertexShell = any ? W.shells.vertexShell.ptr : nullptr;
    out->triShell = any ? W.shells.triShell.ptr : nullptr;
    return PSGPU_RET_SUCCESS;
}

int shells_download(const WeldState& W, PsShell* shells, uint32_t capacity, uint32_t* vertexShell, uint32_t* triShell) {
    const ShellsState& S = W.shells;
    if (!S.valid) return PSGPU_RET_PARAM_ERROR;
    const size_t n = S.info.ctShells, V = S.info.ctVertices, T = S.info.ctTriangles;
    if (shells && capacity < n) return PSGPU_RET_PARAM_ERROR;
    PSGPU_CHECK(download_if(shells, S.shells, n, sizeof(PsShell)));
    PSGPU_CHECK(download_if(vertexShell, S.vertexShell, V, 4));
    PSGPU_CHECK(download_if(triShell, S.triShell, T, 4));
    return PSGPU_RET_SUCCESS;
}

int shells_times(const WeldState& W, float* ms, int maxPhases, const char** names) {
    return W.shells.times.report(ms, maxPhases, names, kShellsPhaseNames);
}

}  // namespace psgpu

using namespace psgpu;

extern "C" {

int psgpu_weld_shells(psgpu_ctx* c, PsShellsInfo* info) {
    if (!ctx_welded(c)) return PSGPU_RET_PARAM_ERROR;
    const int rc = set_device(c);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    return shells_run(c->weld, c->stream, c->timing != 0, info);
}

int psgpu_weld_shells_device(psgpu_ctx* c, PsShellsDevice* out) {
    if (!ctx_welded(c)) return PSGPU_RET_PARAM_ERROR;
    return shells_device(c->weld, out);
}

int psgpu_download_weld_shells(psgpu_ctx* c, PsShell* shells, uint32_t capacity, uint32_t* vertexShell,
                               uint32_t* triShell) {
    if (!ctx_welded(c)) return PSGPU_RET_PARAM_ERROR;
    const int rc = set_device(c);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    return shells_download(c->weld, shells, capacity, vertexShell, triShell);
}

int psgpu_weld_shells_times(psgpu_ctx* c, float* ms, int maxPhases, const char** names) {
    return c ? shells_times(c->weld, ms, maxPhases, names) : 0;
}

}  // extern "C"
