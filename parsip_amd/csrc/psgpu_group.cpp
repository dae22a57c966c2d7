// psgpu_group.cpp — one grid over several devices (C-ABI, include/parsip_gpu.h).
//
// The reference's Polygonize is ONE blocking call that fans the whole MPU list over every
// core (tbb::parallel_for over CMPUProcessor, PS_Polygonizer.cpp:379-382).  The MI355X
// equivalent fans one MPU lattice over the node's GPUs:
//
//   psgpu_group_*   one process, one context per device: contiguous MPU ranges of
//                   near-equal cost (psgpu_split_costs over psgpu_mpu_costs of a planning
//                   run), launched on every device's stream at once; the count exchange is
//                   a host read of each part's totals; psgpu_group_gather assembles the
//                   parts on one device with peer copies over xGMI (hipMemcpyPeerAsync) and
//                   a rebase kernel, or psgpu_group_download_mesh to the host;
//                   psgpu_group_weld welds the gathered parts into one watertight mesh
//                   there (the kernels: psgpu_weld.hip).
//   psgpu_comm_*    one process per GPU, the counts exchanged with RCCL: psgpu_comm.cpp.
//
// What needs no GPU -- the split policy, when polygonize re-splits, the parts' places in the
// whole mesh -- is psgpu_group_plan.h.
//
// MPUs are independent (each evaluates its own 8^3 corners, faces included), so the
// concatenation of the parts in range order IS the single-device mesh: no halo, no
// data-path collective.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "psgpu_group_plan.h"
#include "psgpu_internal.h"
#include "psgpu_launch.h"

using namespace psgpu;

namespace {
constexpr int kGroupWeldPhases = 8;  // psgpu_group_weld_times
const char* kGroupWeldPhaseNames[kGroupWeldPhases] = {
    "group weld total", "gather", "k_weld_edges + copies", "table fill + k_weld_mark_ids",
    "k_weld_resolve",   "k_weld_scan", "k_weld_emit", "k_weld_map"};

using Parts = std::vector<psgpu_ctx*>;

// The gathered mesh (psgpu_group_gather) on one part's device, and the stream that gathers it.
struct Gather {
    int part = -1;
    Stream stream;
    DevBuf<float> pos, nrm, col;
    DevBuf<uint32_t> tris;
    DevBuf<uint64_t> offs;

    void reset(const Parts& parts) {
        if (part < 0) return;
        (void)hipSetDevice(parts[part]->device);
        if (stream) (void)hipStreamSynchronize(stream);
        pos.release();
        nrm.release();
        col.release();
        tris.release();
        offs.release();
        stream.reset();
        part = -1;
    }
};

// One part's edge ids on its own device (k_weld_edges), and the event the gather stream waits for.
struct PartEdges {
    DevBuf<uint64_t> ids;
    Event ready;
};

// The welded mesh on one part's device: allocated by the first weld, grown on demand.
struct GroupWeld {
    int part = -1;
    WeldState state;         // doneSeq: the group's runSeq of the welded run
    DevBuf<uint64_t> gEdge;  // the gathered vertices' edge ids, beside the gathered mesh
    std::vector<PartEdges> edges;  // per part, or none
    PhaseTimes<kGroupWeldPhases> times;

    void reset(const Parts& parts) {
        if (part >= 0) {
            (void)hipSetDevice(parts[part]->device);
            weld_state_free(state);  // (hipFree waits for the device)
            gEdge.release();
            times.free();
        }
        for (size_t p = 0; p < edges.size(); ++p) {
            if (!edges[p].ids && !edges[p].ready) continue;
            (void)hipSetDevice(parts[p]->device);
            edges[p].ids.release();
            edges[p].ready.reset();
        }
        edges.clear();
        part = -1;
    }
};
}  // namespace

struct psgpu_group {
    Parts parts;
    SplitPlan split;
    bool pending = false;
    bool haveResult = false;
    std::vector<PsMeshInfo> info;   // per part, after finish
    std::vector<uint32_t> vBase, tBase;
    PsMeshInfo total{};
    Gather gather;
    // psgpu_group_weld: runSeq counts whatever supersedes the group's run or its split
    // (set_model, polygonize, set_split, a capacity change), as psgpu_ctx::runSeq does for a
    // context; partSeq is each part's own runSeq when the group's finish collected it
    uint64_t runSeq = 0;
    std::vector<uint64_t> partSeq;
    GroupWeld weld;
};

namespace {

uint32_t lattice_total(psgpu_group* g, float cs) {
    uint32_t dims[3] = {0, 0, 0};
    if (psgpu_mpu_dims(cs, &g->parts[0]->primsHost, dims) != PSGPU_RET_SUCCESS) return 0;
    const uint64_t t = (uint64_t)dims[0] * dims[1] * dims[2];
    return t > 0xffffffffull ? 0u : (uint32_t)t;
}

// MPUs per planning run: below the per-run limit (PSGPU_PLAN_CHUNK_MPUS lowers it, so tests
// exercise the chunked plan on small lattices)
uint32_t plan_chunk_mpus() {
    uint32_t chunk = kMaxRangeMpus - 1u;
    if (const char* v = getenv("PSGPU_PLAN_CHUNK_MPUS")) {
        const long x = strtol(v, nullptr, 10);
        if (x > 0 && (uint64_t)x < chunk) chunk = (uint32_t)x;
    }
    return chunk;
}

// Cost split of the lattice from a planning run of the whole grid on part 0 (one
// polygonization per chunk of fewer than kMaxRangeMpus MPUs, the most one run takes;
// results are exact, so every caller that plans the same model and lattice gets the same
// split).
int plan(psgpu_group* g, float cs, uint32_t total) {
    SplitPlan& S = g->split;
    const uint32_t a = S.active_parts(total);
    S.bounds.assign((size_t)S.parts + 1, total);
    S.bounds[0] = 0;
    if (a > 1 && total > 0) {
        std::vector<uint32_t> costs(total);
        // planning runs are not the caller's polygonizations: PrintThreadResults skips them
        g->parts[0]->countThreads = false;
        for (uint32_t b = 0; b < total;) {
            const uint32_t e = (uint32_t)std::min<uint64_t>(total, (uint64_t)b + plan_chunk_mpus());
            int rc = psgpu_polygonize(g->parts[0], cs, b, e, nullptr);
            if (rc == PSGPU_RET_SUCCESS) rc = psgpu_mpu_costs(g->parts[0], costs.data() + b);
            if (rc != PSGPU_RET_SUCCESS) {
                g->parts[0]->countThreads = true;
                return rc;
            }
            b = e;
        }
        g->parts[0]->countThreads = true;
        const int rc = psgpu_split_costs(costs.data(), total, a, 0, S.bounds.data());
        if (rc != PSGPU_RET_SUCCESS) return rc;
    }
    const PsSoaBlobPrims& P = g->parts[0]->primsHost;
    S.planLo = P.bboxLo;
    S.planHi = P.bboxHi;
    S.planCs = cs;
    S.planned = true;
    return PSGPU_RET_SUCCESS;
}

// Re-split from the costs of the run just finished (PSGPU_GROUP_BALANCE_EVERY_RUN).
int replan_from_last(psgpu_group* g) {
    std::vector<uint32_t>& bounds = g->split.bounds;
    const uint32_t n = g->split.parts;
    const uint32_t begin = bounds[0], total = bounds[n] - bounds[0];
    std::vector<uint32_t> costs(total);
    for (uint32_t p = 0; p < n; ++p) {
        if (bounds[p + 1] == bounds[p]) continue;
        const int rc = psgpu_mpu_costs(g->parts[p], costs.data() + (bounds[p] - begin));
        if (rc != PSGPU_RET_SUCCESS) return rc;
    }
    const uint32_t a = g->split.active_parts(total);
    std::fill(bounds.begin(), bounds.end(), begin + total);
    return psgpu_split_costs(costs.data(), total, a, begin, bounds.data());
}

}  // namespace

extern "C" {

int psgpu_group_create(const int* devices, int nParts, psgpu_group** out) {
    if (!out || nParts <= 0 || nParts > 64) return PSGPU_RET_PARAM_ERROR;
    *out = nullptr;
    const int ndev = psgpu_device_count();
    if (ndev <= 0) return PSGPU_RET_DEVICE_ERROR;
    psgpu_group* g = new psgpu_group();
    for (int p = 0; p < nParts; ++p) {
        const int d = devices ? devices[p] : p;
        psgpu_ctx* c = nullptr;
        const int rc = (d >= 0 && d < ndev) ? psgpu_create(d, &c) : PSGPU_RET_DEVICE_ERROR;
        if (rc != PSGPU_RET_SUCCESS) {
            psgpu_group_destroy(g);
            return rc;
        }
        g->parts.push_back(c);
    }
    g->split.parts = (uint32_t)nParts;
    // direct peer access between the parts' devices (xGMI) for the gather; a pair
    // without it still copies (staged by the runtime)
    for (psgpu_ctx* a : g->parts)
        for (psgpu_ctx* b : g->parts) {
            if (a->device == b->device) continue;
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, a->device, b->device) == hipSuccess && can) {
                (void)hipSetDevice(a->device);
                const hipError_t e = hipDeviceEnablePeerAccess(b->device, 0);
                if (e != hipSuccess) (void)hipGetLastError();  // already enabled is fine
            }
        }
    *out = g;
    return PSGPU_RET_SUCCESS;
}

void psgpu_group_destroy(psgpu_group* g) {
    if (!g) return;
    g->weld.reset(g->parts);  // each on its device, ahead of the contexts
    g->gather.reset(g->parts);
    for (psgpu_ctx* c : g->parts) psgpu_destroy(c);
    delete g;
}

int psgpu_group_size(psgpu_group* g) { return g ? (int)g->parts.size() : 0; }

psgpu_ctx* psgpu_group_context(psgpu_group* g, int part) {
    return (g && part >= 0 && part < (int)g->parts.size()) ? g->parts[part] : nullptr;
}

int psgpu_group_set_option(psgpu_group* g, int option, int64_t value) {
    if (!g) return PSGPU_RET_PARAM_ERROR;
    if (option == PSGPU_GROUP_OPT_BALANCE) {
        if (value < 0 || value > 3) return PSGPU_RET_PARAM_ERROR;
        g->split.balance = (int)value;
        g->split.planned = false;
        return PSGPU_RET_SUCCESS;
    }
    if (option == PSGPU_GROUP_OPT_MIN_PART_MPUS) {
        if (value < 0 || value > 0xffffffffll) return PSGPU_RET_PARAM_ERROR;
        g->split.minPartMpus = (uint32_t)value;
        g->split.planned = false;
        g->split.bounds.clear();  // re-split at the next polygonize
        return PSGPU_RET_SUCCESS;
    }
    if (option == PSGPU_OPT_CAPACITY) ++g->runSeq;  // the parts drop their runs
    for (psgpu_ctx* c : g->parts) {
        const int rc = psgpu_set_option(c, option, value);
        if (rc != PSGPU_RET_SUCCESS) return rc;
    }
    return PSGPU_RET_SUCCESS;
}

int psgpu_group_set_model(psgpu_group* g, const PsSoaBlobPrims* prims, const PsSoaPrimMatrices* mats,
                          const PsSoaBlobOps* ops) {
    if (!g) return PSGPU_RET_PARAM_ERROR;
    ++g->runSeq;
    // one hiprtc job serves every part (jit_request dedups by source); each device loads it
    for (psgpu_ctx* c : g->parts) {
        const int rc = psgpu_set_model(c, prims, mats, ops);
        if (rc != PSGPU_RET_SUCCESS) return rc;
    }
    g->haveResult = false;
    return PSGPU_RET_SUCCESS;
}

int psgpu_group_jit_wait(psgpu_group* g) {
    if (!g) return 0;
    int all = 1;
    for (psgpu_ctx* c : g->parts) all &= psgpu_jit_wait(c);
    return all;
}

int psgpu_group_set_split(psgpu_group* g, const uint32_t* bounds) {
    if (!g || !bounds) return PSGPU_RET_PARAM_ERROR;
    const size_t n = g->parts.size();
    for (size_t k = 0; k < n; ++k)
        if (bounds[k] > bounds[k + 1]) return PSGPU_RET_PARAM_ERROR;
    g->split.bounds.assign(bounds, bounds + n + 1);
    g->split.balance = PSGPU_GROUP_BALANCE_FIXED;
    g->split.planned = false;
    ++g->runSeq;
    return PSGPU_RET_SUCCESS;
}

int psgpu_group_get_split(psgpu_group* g, uint32_t* bounds) {
    if (!g || !bounds || !g->split.have_bounds()) return PSGPU_RET_PARAM_ERROR;
    std::copy(g->split.bounds.begin(), g->split.bounds.end(), bounds);
    return PSGPU_RET_SUCCESS;
}

int psgpu_group_polygonize(psgpu_group* g, float cellsize) {
    if (!g || !g->parts[0]->haveModel || !(cellsize > 0.0f)) return PSGPU_RET_PARAM_ERROR;
    ++g->runSeq;
    const uint32_t total = lattice_total(g, cellsize);
    const size_t n = g->parts.size();
    const PsSoaBlobPrims& P = g->parts[0]->primsHost;
    const SplitDecision d = decide(g->split, cellsize, P.bboxLo, P.bboxHi, total, g->pending);
    if (d.finishFirst) {
        // the split depends on the previous run: finish it first (else runs queue up per
        // part stream, each context double-buffers its counters)
        PsMeshInfo tmp;
        const int rc = psgpu_group_finish(g, &tmp, nullptr);
        if (rc != PSGPU_RET_SUCCESS) return rc;
    }
    if (d.action == SplitAction::Even) {
        g->split.even_split(total);
    } else if (d.action == SplitAction::Plan) {
        const int rc = plan(g, cellsize, total);
        if (rc != PSGPU_RET_SUCCESS) return rc;
    }
    // every device gets its range at once: the launches are asynchronous, per device stream
    const std::vector<uint32_t>& bounds = g->split.bounds;
    for (size_t p = 0; p < n; ++p) {
        const int rc = psgpu_polygonize(g->parts[p], cellsize, bounds[p], bounds[p + 1], nullptr);
        if (rc != PSGPU_RET_SUCCESS) return rc;
    }
    g->pending = true;
    g->haveResult = false;
    return PSGPU_RET_SUCCESS;
}

int psgpu_group_finish(psgpu_group* g, PsMeshInfo* totalOut, PsGroupPart* partsOut) {
    if (!g) return PSGPU_RET_PARAM_ERROR;
    const size_t n = g->parts.size();
    if (g->pending) {
        g->pending = false;
        g->info.assign(n, PsMeshInfo{});
        g->partSeq.assign(n, ~0ull);
        for (size_t p = 0; p < n; ++p) {
            const int rc = psgpu_finish(g->parts[p], &g->info[p]);
            if (rc != PSGPU_RET_SUCCESS) return rc;
            g->partSeq[p] = g->parts[p]->runSeq;
        }
        // the count exchange: each part's place in the global index space
        g->vBase.assign(n, 0);
        g->tBase.assign(n, 0);
        const int placed = place_parts(g->info.data(), n, g->vBase.data(), g->tBase.data(), &g->total);
        if (placed != PSGPU_RET_SUCCESS) return placed;
        g->haveResult = true;
        if (g->split.balance == PSGPU_GROUP_BALANCE_EVERY_RUN && n > 1) {
            const int rc = replan_from_last(g);
            if (rc != PSGPU_RET_SUCCESS) return rc;
        }
    }
    if (!g->haveResult) return PSGPU_RET_PARAM_ERROR;
    if (totalOut) *totalOut = g->total;
    if (partsOut) {
        for (size_t p = 0; p < n; ++p) {
            PsGroupPart& P = partsOut[p];
            P.device = g->parts[p]->device;
            P.mpuBegin = g->parts[p]->mpuBegin;
            P.mpuEnd = g->parts[p]->mpuBegin + g->parts[p]->mpuCount;
            P.vertexBase = g->vBase[p];
            P.triangleBase = g->tBase[p];
            P.info = g->info[p];
        }
    }
    return PSGPU_RET_SUCCESS;
}

// The whole mesh on the host, exactly as one device would produce it: part p's
// vertices at its vertex base, its triangle ids and MPU offsets rebased.
int psgpu_group_download_mesh(psgpu_group* g, float* pos, float* nrm, float* col, uint32_t* tris,
                              uint64_t* mpuOffsets) {
    PsMeshInfo T;
    int rc = psgpu_group_finish(g, &T, nullptr);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    const size_t n = g->parts.size();
    std::vector<OffsetRebase> rebase(n);
    const bool anyMpu = offset_rebases(g->info.data(), g->vBase.data(), g->tBase.data(), n, rebase.data());
    std::vector<uint64_t> offs;
    for (size_t p = 0; p < n; ++p) {
        const PsMeshInfo& I = g->info[p];
        const size_t vb = g->vBase[p], tb = g->tBase[p];
        offs.assign((size_t)I.ctMPUs + 1, 0);
        rc = psgpu_download_mesh(g->parts[p], pos ? pos + vb * 3 : nullptr, nrm ? nrm + vb * 3 : nullptr,
                                 col ? col + vb * 3 : nullptr, tris ? tris + tb * 3 : nullptr, offs.data());
        if (rc != PSGPU_RET_SUCCESS) return rc;
        if (tris)
            for (size_t i = tb * 3; i < (tb + I.ctTriangles) * 3; ++i) tris[i] += (uint32_t)vb;
        if (mpuOffsets)
            for (size_t i = 0; i <= I.ctMPUs; ++i) mpuOffsets[rebase[p].mBase + i] = offs[i] + rebase[p].add;
    }
    if (mpuOffsets && !anyMpu) mpuOffsets[0] = 0;
    return PSGPU_RET_SUCCESS;
}

// The gather of the finished run (totals T) enqueued on the gather stream of dstPart's device,
// which it leaves current; `before` (or null): an event recorded on that stream first.
static int gather_enqueue(psgpu_group* g, int dstPart, const PsMeshInfo& T, hipEvent_t before) {
    int rc;
    Gather& G = g->gather;
    if (G.part != dstPart) G.reset(g->parts);
    psgpu_ctx* dst = g->parts[dstPart];
    PSGPU_CHECK(hipSetDevice(dst->device));
    PSGPU_CHECK(G.stream.create(hipStreamNonBlocking));
    G.part = dstPart;
    if (before) PSGPU_CHECK(hipEventRecord(before, G.stream));
    const size_t V = std::max<size_t>(T.ctVertices, 1), Tn = std::max<size_t>(T.ctTriangles, 1),
                 M = (size_t)T.ctMPUs + 1;
    PSGPU_CHECK(G.pos.reserve(V * 3, Growth::Exact));
    PSGPU_CHECK(G.nrm.reserve(V * 3, Growth::Exact));
    PSGPU_CHECK(G.col.reserve(V * 3, Growth::Exact));
    PSGPU_CHECK(G.tris.reserve(Tn * 3, Growth::Exact));
    PSGPU_CHECK(G.offs.reserve(M, Growth::Exact));
    hipStream_t s = G.stream;
    const size_t n = g->parts.size();
    std::vector<OffsetRebase> rebase(n);
    const bool anyMpu = offset_rebases(g->info.data(), g->vBase.data(), g->tBase.data(), n, rebase.data());
    for (size_t p = 0; p < n; ++p) {
        psgpu_ctx* c = g->parts[p];
        const PsMeshInfo& I = g->info[p];
        PsMeshDevice src;
        rc = psgpu_mesh_device(c, &src);
        if (rc != PSGPU_RET_SUCCESS) return rc;
        PSGPU_CHECK(hipSetDevice(dst->device));
        const size_t vb = g->vBase[p], tb = g->tBase[p];
        const int sd = c->device, dd = dst->device;
        uint64_t* offs = G.offs + rebase[p].mBase;
        if (I.ctVertices) {
            PSGPU_CHECK(hipMemcpyPeerAsync(G.pos + vb * 3, dd, src.pos, sd, (size_t)I.ctVertices * 12, s));
            PSGPU_CHECK(hipMemcpyPeerAsync(G.nrm + vb * 3, dd, src.nrm, sd, (size_t)I.ctVertices * 12, s));
            PSGPU_CHECK(hipMemcpyPeerAsync(G.col + vb * 3, dd, src.col, sd, (size_t)I.ctVertices * 12, s));
        }
        if (I.ctTriangles)
            PSGPU_CHECK(hipMemcpyPeerAsync(G.tris + tb * 3, dd, src.tris, sd, (size_t)I.ctTriangles * 12, s));
        if (I.ctMPUs) PSGPU_CHECK(hipMemcpyPeerAsync(offs, dd, src.mpuOffsets, sd, ((size_t)I.ctMPUs + 1) * 8, s));
        PSGPU_CHECK(launch_rebase(G.tris + tb * 3, (uint64_t)I.ctTriangles * 3, (uint32_t)vb, offs,
                                  I.ctMPUs ? (uint64_t)I.ctMPUs + 1 : 0, rebase[p].add, s));
    }
    if (!anyMpu) PSGPU_CHECK(hipMemsetAsync(G.offs, 0, 8, s));
    return PSGPU_RET_SUCCESS;
}

// The whole mesh in HBM of one part's device: peer copies of every part (xGMI), then the
// rebase kernel per part.  The returned pointers stay valid until the next gather.
int psgpu_group_gather(psgpu_group* g, int dstPart, PsMeshDevice* out) {
    if (!g || !out || dstPart < 0 || dstPart >= (int)g->parts.size()) return PSGPU_RET_PARAM_ERROR;
    PsMeshInfo T;
    int rc = psgpu_group_finish(g, &T, nullptr);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    rc = gather_enqueue(g, dstPart, T, nullptr);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    const Gather& G = g->gather;
    PSGPU_CHECK(hipStreamSynchronize(G.stream));
    out->pos = G.pos;
    out->nrm = G.nrm;
    out->col = G.col;
    out->tris = G.tris;
    out->mpuOffsets = G.offs;
    return PSGPU_RET_SUCCESS;
}

// The group's run welded as one mesh on dstPart's device (psgpu_weld's contract over the
// gathered index space): every part turns its vertex records into edge ids on its own device
// and stream (k_weld_edges), the gather stream gathers the mesh, waits for each part's event
// and copies its ids behind the previous part's, then marks from the ids and runs the
// context weld's resolve / scan / emit / map on the gathered arrays.
int psgpu_group_weld(psgpu_group* g, int dstPart, PsWeldInfo* info) {
    if (!g || dstPart < 0 || dstPart >= (int)g->parts.size()) return PSGPU_RET_PARAM_ERROR;
    PsMeshInfo T;
    int rc = psgpu_group_finish(g, &T, nullptr);  // PSGPU_RET_PARAM_ERROR without a run
    if (rc != PSGPU_RET_SUCCESS) return rc;
    if (T.firstOverflowMPU >= 0) return PSGPU_RET_PARAM_ERROR;  // past the reference's 512 per MPU
    const size_t n = g->parts.size();
    for (size_t p = 0; p < n; ++p) {
        const psgpu_ctx* c = g->parts[p];
        // the part still holds the run the group collected (not one made through its own pointer)
        if (!weld_run_ready(c) || c->runSeq != g->partSeq[p]) return PSGPU_RET_PARAM_ERROR;
        if (!weld_lattice_fits(c->dims)) return PSGPU_RET_PARAM_ERROR;
    }
    GroupWeld& GW = g->weld;
    if (GW.part != dstPart) GW.reset(g->parts);
    GW.part = dstPart;
    WeldState& W = GW.state;
    PhaseTimes<kGroupWeldPhases>& times = GW.times;
    times.clear();
    if (!weld_begin(W, T.ctVertices, T.ctTriangles, g->runSeq, info)) return PSGPU_RET_SUCCESS;
    if (GW.edges.size() != n) GW.edges.resize(n);  // (empty before: reset clears them)
    // the parts' edge ids, each on its own device and stream: devices work side by side
    for (size_t p = 0; p < n; ++p) {
        psgpu_ctx* c = g->parts[p];
        if (!g->info[p].ctVertices) continue;
        rc = set_device(c);
        if (rc != PSGPU_RET_SUCCESS) return rc;
        PartEdges& E = GW.edges[p];
        PSGPU_CHECK(E.ids.reserve(g->info[p].ctVertices, Growth::ByHalf));
        PSGPU_CHECK(E.ready.create(hipEventDisableTiming));
        rc = weld_edges(c, E.ids, c->stream);
        if (rc != PSGPU_RET_SUCCESS) return rc;
        PSGPU_CHECK(hipEventRecord(E.ready, c->stream));
    }
    psgpu_ctx* dst = g->parts[dstPart];
    PSGPU_CHECK(hipSetDevice(dst->device));
    PSGPU_CHECK(times.begin(dst->timing != 0));
    PSGPU_CHECK(GW.gEdge.reserve(T.ctVertices, Growth::ByHalf));
    rc = gather_enqueue(g, dstPart, T, times.take());
    if (rc != PSGPU_RET_SUCCESS) return rc;
    const Gather& G = g->gather;
    hipStream_t s = G.stream;
    PSGPU_CHECK(times.mark(s));
    for (size_t p = 0; p < n; ++p) {
        if (!g->info[p].ctVertices) continue;
        PSGPU_CHECK(hipStreamWaitEvent(s, GW.edges[p].ready, 0));
        PSGPU_CHECK(hipMemcpyPeerAsync(GW.gEdge + g->vBase[p], dst->device, GW.edges[p].ids, g->parts[p]->device,
                                       (size_t)g->info[p].ctVertices * sizeof(uint64_t), s));
    }
    // the mark that ends the copies' phase is weld_enqueue's first
    const WeldInput in{G.pos, G.nrm, G.col, G.tris, T.ctVertices, T.ctTriangles, GW.gEdge, nullptr};
    rc = weld_enqueue(W, in, s, times.rest());
    if (rc == PSGPU_RET_SUCCESS) rc = weld_end(W, s, g->runSeq, info);
    if (rc == PSGPU_RET_SUCCESS) times.collect();
    return rc;
}

// the group's current run has been welded
static bool group_welded(const psgpu_group* g) {
    return g && g->haveResult && !g->pending && g->weld.part >= 0 && g->weld.state.doneSeq == g->runSeq;
}

// ... and its device is current: what the entry points below that work there start from.  *stream:
// the gather stream the weld ran on (the part's own after a weld of an empty mesh, which made
// none); *timed: the welding part's PSGPU_OPT_KERNEL_TIMING.
static int welded_target(const psgpu_group* g, hipStream_t* stream = nullptr, bool* timed = nullptr) {
    if (!group_welded(g)) return PSGPU_RET_PARAM_ERROR;
    const psgpu_ctx* dst = g->parts[g->weld.part];
    PSGPU_CHECK(hipSetDevice(dst->device));
    if (stream) *stream = g->gather.stream ? (hipStream_t)g->gather.stream : (hipStream_t)dst->stream;
    if (timed) *timed = dst->timing != 0;
    return PSGPU_RET_SUCCESS;
}

int psgpu_group_weld_device(psgpu_group* g, PsWeldDevice* out) {
    if (!out || !group_welded(g)) return PSGPU_RET_PARAM_ERROR;
    return weld_device(g->weld.state, out);
}

int psgpu_group_download_weld(psgpu_group* g, float* pos, float* nrm, float* col, uint32_t* tris,
                              uint32_t* vertexMap) {
    const int rc = welded_target(g);
    return rc != PSGPU_RET_SUCCESS ? rc : weld_download(g->weld.state, pos, nrm, col, tris, vertexMap);
}

int psgpu_group_weld_times(psgpu_group* g, float* ms, int maxPhases, const char** names) {
    return g ? g->weld.times.report(ms, maxPhases, names, kGroupWeldPhaseNames) : 0;
}

// The shells of the group's weld (psgpu_shells.hip), on the welding part's device and the
// gather stream the weld ran on.
int psgpu_group_weld_shells(psgpu_group* g, PsShellsInfo* info) {
    hipStream_t s;
    bool timed;
    const int rc = welded_target(g, &s, &timed);
    return rc != PSGPU_RET_SUCCESS ? rc : shells_run(g->weld.state, s, timed, info);
}

int psgpu_group_weld_shells_device(psgpu_group* g, PsShellsDevice* out) {
    if (!group_welded(g)) return PSGPU_RET_PARAM_ERROR;
    return shells_device(g->weld.state, out);
}

int psgpu_group_download_weld_shells(psgpu_group* g, PsShell* shells, uint32_t capacity, uint32_t* vertexShell,
                                     uint32_t* triShell) {
    const int rc = welded_target(g);
    return rc != PSGPU_RET_SUCCESS ? rc : shells_download(g->weld.state, shells, capacity, vertexShell, triShell);
}

int psgpu_group_weld_shells_times(psgpu_group* g, float* ms, int maxPhases, const char** names) {
    return g ? shells_times(g->weld.state, ms, maxPhases, names) : 0;
}

// The filter of the group's weld by its shells (psgpu_filter.hip), where the shells ran.
int psgpu_group_weld_filter(psgpu_group* g, const PsShellFilter* f, const uint8_t* mask, uint32_t maskCount,
                            PsFilterInfo* info) {
    hipStream_t s;
    bool timed;
    const int rc = welded_target(g, &s, &timed);
    return rc != PSGPU_RET_SUCCESS ? rc : filter_run(g->weld.state, s, timed, f, mask, maskCount, info);
}

int psgpu_group_weld_filter_device(psgpu_group* g, PsFilterDevice* out) {
    if (!group_welded(g)) return PSGPU_RET_PARAM_ERROR;
    return filter_device(g->weld.state, out);
}

int psgpu_group_download_weld_filter(psgpu_group* g, float* pos, float* nrm, float* col, uint32_t* tris,
                                     uint32_t* vertexMap, uint32_t* shellMap, PsShell* shells,
                                     uint32_t shellCapacity) {
    const int rc = welded_target(g);
    return rc != PSGPU_RET_SUCCESS ? rc
                                   : filter_download(g->weld.state, pos, nrm, col, tris, vertexMap, shellMap, shells,
                                                     shellCapacity);
}

int psgpu_group_weld_filter_times(psgpu_group* g, float* ms, int maxPhases, const char** names) {
    return g ? filter_times(g->weld.state, ms, maxPhases, names) : 0;
}

int psgpu_group_export_polympus(psgpu_group* g, PsMPU* mpus, uint32_t capacity, uint32_t* outCt) {
    PsMeshInfo T;
    int rc = psgpu_group_finish(g, &T, nullptr);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    if (outCt) *outCt = T.ctMPUs;
    if (T.ctMPUs > capacity) return PSGPU_RET_MPU_OVERFLOW;
    if (T.firstOverflowMPU >= 0) return PSGPU_RET_MPU_VT_OVERFLOW;
    if (!mpus) return PSGPU_RET_PARAM_ERROR;
    // every part's packing first (each on its own stream)
    std::vector<ExportStage> st(g->parts.size());
    for (size_t p = 0; p < g->parts.size(); ++p) {
        rc = set_device(g->parts[p]);
        // parts on one device share its link: each part's packing waits for the previous
        // part's, so the pieces arrive in range order, as the scatter threads take them
        hipEvent_t after =
            p > 0 && g->parts[p - 1]->device == g->parts[p]->device ? g->parts[p - 1]->exportEv[1] : nullptr;
        if (rc == PSGPU_RET_SUCCESS) rc = export_stage(g->parts[p], true, false, &st[p], after);
        if (rc != PSGPU_RET_SUCCESS) return rc;
    }
    // then one pass of the first part's scatter threads over every part, in range order per
    // thread: the parts' packing kernels share the link, the threads follow them
    std::vector<ScatterJob> jobs(g->parts.size());
    uint32_t at = 0;
    for (size_t p = 0; p < g->parts.size(); ++p) {
        rc = jobs[p].prepare(g->parts[p], st[p], mpus + at);
        if (rc != PSGPU_RET_SUCCESS) return rc;
        at += g->parts[p]->mpuCount;
    }
    rc = scatter_jobs(g->parts[0], jobs.data(), jobs.size());
    for (size_t p = 0; p < g->parts.size() && rc == PSGPU_RET_SUCCESS; ++p) {
        rc = set_device(g->parts[p]);
        if (rc == PSGPU_RET_SUCCESS) rc = jobs[p].finish(nullptr);
    }
    return rc;
}

int psgpu_group_polygonize_mpus(psgpu_group* g, float cellsize, const PsSoaBlobPrims* prims,
                                const PsSoaPrimMatrices* mats, const PsSoaBlobOps* ops, PsMPU* mpus,
                                uint32_t capacity, uint32_t* outCt) {
    if (!g || !prims) return PSGPU_RET_PARAM_ERROR;
    if (prims->ctPrims == 0) return PSGPU_RET_PARAM_ERROR;  // Polygonize :322-323
    int rc = psgpu_group_set_model(g, prims, mats, ops);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    rc = psgpu_group_polygonize(g, cellsize);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    return psgpu_group_export_polympus(g, mpus, capacity, outCt);
}

}  // extern "C"
