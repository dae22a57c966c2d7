// psgpu_host.cpp — C-ABI of the MI355X polygonizer (include/parsip_gpu.h).
//
// Host side of PS::SIMDPOLY::Polygonize (PS_Polygonizer.cpp:315-385): MPU lattice,
// model upload (the reference's per-thread FieldComputer copy, :22-50, becomes one
// 28 KB device image read through the scalar cache), kernel sequencing on one HIP
// stream, the verdict on each finished run and the diagnostic downloads.  What needs no GPU is
// decided elsewhere: the model image in psgpu_model_build.h, a run's launch shape and its verdict
// in psgpu_plan.h; the blocking export back to the reference's PolyMPUs is psgpu_export.cpp.
#include <hip/hip_runtime.h>

#include <atomic>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/parsip_gpu.h"
#include "psgpu_internal.h"
#include "psgpu_launch.h"
#include "psgpu_model_build.h"

using namespace psgpu;

namespace {

const char* kKernelNames[kNumKernels] = {"k_precheck", "k_mpu", "k_vertex", "k_finish"};

}  // namespace

namespace psgpu {
int hip_fail(hipError_t e, const char* what) {
    if (e == hipSuccess) return PSGPU_RET_SUCCESS;
    fprintf(stderr, "psgpu: %s failed: %s\n", what, hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? PSGPU_RET_NOT_ENOUGH_MEM : PSGPU_RET_DEVICE_ERROR;
}

int set_device(psgpu_ctx* c) { return hip_fail(hipSetDevice(c->device), "hipSetDevice"); }

int finished_run(psgpu_ctx* c, PsMeshInfo* info) {
    const int rc = psgpu_finish(c, info);  // PARAM_ERROR for a null context
    return rc == PSGPU_RET_SUCCESS ? set_device(c) : rc;
}
}  // namespace psgpu

namespace {

// The brick layout of the context's range: computed once per enqueue and handed to what sizes the
// buffers, plans the run and fills its parameters.
BrickLayout run_bricks(const psgpu_ctx* c) { return brick_layout(c->dims, c->mpuBegin, c->mpuCount); }

// The context's four capacities as psgpu_plan.h judges and grows them.
Caps caps_of(const psgpu_ctx* c) { return {c->vcap, c->tcap, c->vShardCap, c->tShardCap}; }
void set_caps(psgpu_ctx* c, const Caps& k) {
    c->vcap = k.v;
    c->tcap = k.t;
    c->vShardCap = k.shardV;
    c->tShardCap = k.shardT;
}

int ensure_buffers(psgpu_ctx* c, const BrickLayout& bricks) {
    const size_t n = std::max<uint32_t>(c->mpuCount, 1);
    const size_t nBricks = brick_count(bricks);
    c->pShardCap = 8u * (uint32_t)((nBricks + kShards - 1) / kShards);
    // k_front's 8 sub-queues: a block's bricks x 8 MPUs for every 8th k_precheck block
    const size_t fq = 8 * front_cap(nBricks);
    const size_t nq = std::max<size_t>((size_t)c->pShardCap * kShards, fq);
    constexpr Growth H = Growth::ByHalf;
    PSGPU_CHECK(c->pq.reserve(nq, H));
    PSGPU_CHECK(c->pqMask.reserve(nq * 4, H));  // culling + op-inside mask per entry
    PSGPU_CHECK(c->liveList.reserve(nBricks, H));  // k_sieve: at most every brick
    bool fresh = false;
    if (fq) PSGPU_CHECK(c->fqReady.reserve(fq, H, &fresh));
    if (fresh)  // ready words start at 0: no run's tag
        PSGPU_CHECK(hipMemset(c->fqReady, 0, c->fqReady.cap * sizeof(uint32_t)));
    PSGPU_CHECK(c->counts.reserve(n, H));
    PSGPU_CHECK(c->passed.reserve(n, H));
    PSGPU_CHECK(c->mpuMasks.reserve(4 * n, H));
    PSGPU_CHECK(c->offs.reserve(n + 1, H));
    PSGPU_CHECK(c->vk.reserve((size_t)c->vShardCap * kShards, H));
    PSGPU_CHECK(c->vp.reserve((size_t)c->vShardCap * kShards, H));
    PSGPU_CHECK(c->tq.reserve((size_t)c->tShardCap * kShards, H));
    PSGPU_CHECK(c->pos.reserve((size_t)c->vcap * 3, H));
    PSGPU_CHECK(c->nrm.reserve((size_t)c->vcap * 3, H));
    PSGPU_CHECK(c->col.reserve((size_t)c->vcap * 3, H));
    PSGPU_CHECK(c->tris.reserve((size_t)c->tcap * 3, H));
    if (c->mpuTicksOpt) PSGPU_CHECK(c->mpuTicks.reserve(4 * n, H));
    return PSGPU_RET_SUCCESS;
}

// The launch shape of the context's next run (psgpu_plan.h decides it, from these inputs alone).
// separate: finish re-runs a run whose in-kernel wait gave up, as separate launches.
LaunchPlan plan_run(const psgpu_ctx* c, const BrickLayout& bricks, bool separate) {
    PlanInput in{};
    in.numCUs = c->numCUs;
    in.bricks = brick_count(bricks);
    in.mpuCount = c->mpuCount;
    in.opt = c->opt;
    in.last = c->last;
    in.alone = c->alone;
    in.crowded = c->crowded;
    in.mpuTicks = c->mpuTicksOpt != 0;
    in.splittable = c->splittable;
    // k_sieve: with culling on, a root-zero set, and brick coordinates that fit a list entry
    const uint32_t* bd = bricks.dims;
    in.sievable = c->cull != 0 && c->model.rootZeroValid != 0u && (uint64_t)bricks.i0 + bd[0] <= (1u << 21) &&
                  bd[1] <= (1u << 21) && bd[2] <= (1u << 21);
    if (const JitKernels* J = c->jit.kernels.get()) {
        in.jit = true;
        in.hasPrecheckS = J->precheckS != nullptr;
        in.hasSurface = J->surface != nullptr;
        in.hasSurfaceW = J->surfaceW != nullptr;
        in.hasFront = J->front != nullptr;
        in.hasFrontS = J->frontS != nullptr;
    }
    in.separate = separate;
    in.shortGrid = (c->debug & (1 << 20)) != 0;
    return plan_launch(in);
}

Params make_params(psgpu_ctx* c, const BrickLayout& bricks, const LaunchPlan& plan) {
    Params p;
    memset(&p, 0, sizeof(p));  // padding too: graph replay compares parameter bytes
    p.model = c->dModel;
    p.tables = c->dTables;
    p.cs = c->cs;
    p.side = c->cs * (float)PSGPU_CELLS_PER_MPU;
    p.lo[0] = c->primsHost.bboxLo.x;
    p.lo[1] = c->primsHost.bboxLo.y;
    p.lo[2] = c->primsHost.bboxLo.z;
    for (int a = 0; a < 3; ++a) p.dims[a] = c->dims[a];
    p.divMagic[0] = p.dims[2] ? 0xffffffffu / p.dims[2] : 0u;
    p.divMagic[1] = (p.dims[2] * p.dims[1]) ? 0xffffffffu / (p.dims[2] * p.dims[1]) : 0u;
    p.mpuBegin = c->mpuBegin;
    p.mpuCount = c->mpuCount;
    p.cull = (uint32_t)c->cull;
    p.brickI0 = bricks.i0;
    for (int a = 0; a < 3; ++a) p.brickDims[a] = bricks.dims[a];
    p.preBlocks = plan.preBlocks;
    p.brickStride = brick_stride((uint32_t)brick_count(bricks), (c->debug & 16384) != 0);
    p.brickMagic[0] = p.brickDims[2] ? 0xffffffffu / p.brickDims[2] : 0u;
    p.brickMagic[1] = (p.brickDims[2] * p.brickDims[1]) ? 0xffffffffu / (p.brickDims[2] * p.brickDims[1]) : 0u;
    p.sieve = plan.sieve;
    p.liveList = c->liveList;
    p.pq = c->pq;
    p.pqMask = c->pqMask;
    p.pShardCap = c->pShardCap;
    p.mpuBlocks = plan.mpuBlocks;
    p.fqReady = c->fqReady;
    p.fqCap = plan.fqCap;
    p.scanChunks = plan.scanChunks;
    p.scanBlocks = plan.scanBlocks;
    p.scanStatus = c->scanStatus + (size_t)c->parity * kScanMaxBlocks;
    p.scanStatusNext = c->scanStatus + (size_t)(c->parity ^ 1u) * kScanMaxBlocks;
    p.counts = c->counts;
    p.passed = c->passed;
    p.bound = (c->bound && c->jit.kernels && c->model.boundable) ? 1u : 0u;
    p.opInside = c->opInside ? 1u : 0u;
    p.mpuMasks = c->mpuMasks;
    p.offs = c->offs;
    p.vk = c->vk;
    p.vp = c->vp;
    p.vShardCap = c->vShardCap;
    p.tq = c->tq;
    p.tShardCap = c->tShardCap;
    p.pos = c->pos;
    p.nrm = c->nrm;
    p.col = c->col;
    p.tris = c->tris;
    p.vCap = c->vcap;
    p.tCap = c->tcap;
    p.ctr = c->ctr + c->parity;
    p.ctrNext = c->ctr + (c->parity ^ 1u);
    p.hostCtr = c->hostCtrDev;
    p.totals = c->totals;
    p.stamps = c->stamps;
    p.stampCap = c->stamps ? c->stampCap : 0u;
    p.spans = (c->spans && c->spanNext < c->spanCap)
                  ? c->spans + (size_t)c->spanNext * 2 * kNumStampKernels * kSpanLanes : nullptr;
    p.mpuTicks = c->mpuTicksOpt ? c->mpuTicks : nullptr;
    p.slotsPerLane = c->jit.kernels ? 0u : c->model.nSlots;
    p.debug = (uint32_t)c->debug;
    return p;
}

hipError_t launch_jit(hipFunction_t f, uint32_t blocks, uint32_t threads, size_t lds, hipStream_t s, Params& p) {
    void* args[] = {&p};
    return hipModuleLaunchKernel(f, blocks, 1, 1, threads, 1, 1, (unsigned)lds, s, args, nullptr);
}

// The launches of one polygonization as the plan shapes them (shared by direct launch and
// graph capture): k_precheck and k_mpu, or both as k_front, then k_vertex and k_finish, or both
// as k_surface.  No copies or fills.
int launch_all(psgpu_ctx* c, const Params& pin, const LaunchPlan& plan, hipStream_t s, bool timed) {
    Params p = pin;
    JitKernels* J = c->jit.kernels.get();
    // the split kernel's blocks hold 2 MPUs, the others 4 (mpu_lds_bytes(0): 4 MPUs' LDS)
    const size_t mpuLds = mpu_lds_bytes(0) / (plan.split ? 2 : 1);
    if (timed) PSGPU_CHECK(hipEventRecord(c->ev[0], s));
    if (plan.sieve) PSGPU_CHECK(launch_sieve(p, s));  // ahead of S1; counted with k_precheck's time
    if (plan.front) {  // S1 blocks, then S2 blocks taking the survivors as they are published
        PSGPU_CHECK(launch_jit(plan.split ? J->frontS : J->front, plan.preBlocks + plan.mpuBlocks, 256, mpuLds, s, p));
        if (timed) {
            PSGPU_CHECK(hipEventRecord(c->ev[1], s));
            PSGPU_CHECK(hipEventRecord(c->ev[2], s));
        }
    } else {
        if (J) PSGPU_CHECK(launch_jit(plan.split ? J->precheckS : J->precheck, plan.preBlocks, 256, 0, s, p));
        else PSGPU_CHECK(launch_precheck(p, s));
        if (timed) PSGPU_CHECK(hipEventRecord(c->ev[1], s));
        if (J) PSGPU_CHECK(launch_jit(plan.split ? J->mpuS : J->mpu, plan.mpuBlocks, 256, mpuLds, s, p));
        else PSGPU_CHECK(launch_mpu(p, s));
        if (timed) PSGPU_CHECK(hipEventRecord(c->ev[2], s));
    }
    // k_vertex's (k_surface's) first scanBlocks blocks also compute the mesh offsets
    if (plan.surface) {
        PSGPU_CHECK(launch_jit(plan.surfaceWide ? J->surfaceW : J->surface, plan.gridSurface, 256, 0, s, p));
        if (timed) {
            PSGPU_CHECK(hipEventRecord(c->ev[3], s));
            PSGPU_CHECK(hipEventRecord(c->ev[4], s));
        }
        return PSGPU_RET_SUCCESS;
    }
    if (J) PSGPU_CHECK(launch_jit(plan.vpwVertex == 64 ? J->vertexW : J->vertex, plan.gridVertex, 256, 0, s, p));
    else PSGPU_CHECK(launch_vertex(p, s, plan.gridVertex));
    if (timed) PSGPU_CHECK(hipEventRecord(c->ev[3], s));
    const uint32_t vpw = plan.vpwFinish;
    if (J) PSGPU_CHECK(launch_jit(vpw == 16 ? J->finishQ : (vpw == 32 ? J->finishP : J->finish), plan.gridFinish, 256, 0, s, p));
    else PSGPU_CHECK(launch_finish(p, s, plan.gridFinish, (int)vpw));
    if (timed) PSGPU_CHECK(hipEventRecord(c->ev[4], s));
    return PSGPU_RET_SUCCESS;
}

void drop_graphs(psgpu_ctx* c) {
    for (auto& g : c->graphs) {
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
        g = psgpu_ctx::GraphSlot{};
    }
}

// Ahead of a change to what a run or a captured graph uses: wait for the pending run, drop the graphs.
void quiesce(psgpu_ctx* c) {
    if (c->pending) (void)hipStreamSynchronize(c->runStream);
    drop_graphs(c);
}

// The counters of a run that found nothing: all zero, no overflow.
DevCounters empty_counters() {
    DevCounters d{};
    d.firstOverflow = 0x7fffffff;
    return d;
}

// The stamp buffer of `cap` waves a kernel (PSGPU_OPT_STAMPS): 24 bytes a wave per kernel, then 64 a wave.
size_t stamp_bytes(size_t cap) { return (size_t)kNumStampKernels * cap * 24 + cap * 64; }

// Enqueue one polygonization: its shape is planned once, here, and kept as c->run.  k_precheck
// needs nothing reset (k_finish of the previous run reset this run's counters) and k_finish
// publishes the counters to mapped host memory.  Replayed from a hipGraph (one per counter
// set) while the kernels, the parameters and the plan repeat, e.g. per frame of an animation.
// separate: a protocol-error re-run, as separate launches.
void reset_run_state(psgpu_ctx* c);
int enqueue(psgpu_ctx* c, hipStream_t s, const BrickLayout& bricks, bool separate = false) {
    if (c->mpuCount == 0) {  // nothing to launch: an empty result
        c->runTicks = c->mpuTicksOpt != 0;
        *c->hostCtr = empty_counters();
        // the totals the count exchange reads (k_finish writes them on a real run): zero
        // MPUs, no overflow -- never a previous run's
        PSGPU_CHECK(hipMemcpyAsync(c->totals, c->emptyTotals, 8 * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
        return PSGPU_RET_SUCCESS;
    }
    if (c->debug & (1 << 28)) {  // test hook: 3 runs short of the epoch's wrap
        c->debug &= ~(1 << 28);
        reset_run_state(c);
        DevCounters near;
        PSGPU_CHECK(hipMemcpy(&near, c->ctr, sizeof(DevCounters), hipMemcpyDeviceToHost));
        near.epoch = 0xfffffffcu;
        PSGPU_CHECK(hipMemcpy(c->ctr, &near, sizeof(DevCounters), hipMemcpyHostToDevice));
        c->epochRuns = near.epoch;
    }
    // a run at epoch 0xffffffff would tag k_front's entries 0, the value of ready words no run
    // has written: restart the counter sets at epoch 0 with the ready words zeroed (a stream
    // drain once in 2^32 runs)
    if (c->epochRuns >= 0xffffffffull) reset_run_state(c);
    ++c->epochRuns;
    const LaunchPlan plan = c->run = plan_run(c, bricks, separate);
    const Params p = make_params(c, bricks, plan);
    c->runTicks = p.mpuTicks != nullptr;
    c->debug &= ~((1 << 20) | (1 << 25) | (1 << 26) | (1 << 27));  // the short-grid / protocol test hooks apply to one run
    if (p.spans) c->spanNext++;
    const uint32_t slot = c->parity;
    c->parity ^= 1u;  // k_finish of this run resets the other set for the next run
    const bool timed = c->timing != 0;
    if (c->stamps)  // waves that do not run leave no stale records
        PSGPU_CHECK(hipMemsetAsync(c->stamps, 0, stamp_bytes(c->stampCap), s));
    if (!c->useGraph || timed || s == nullptr) {
        const int rc = launch_all(c, p, plan, s, timed);
        if (rc != PSGPU_RET_SUCCESS) reset_run_state(c);
        return rc;
    }
    psgpu_ctx::GraphSlot& g = c->graphs[slot];
    if (!(g.exec && g.jit == c->jit.kernels.get() && memcmp(&g.key, &p, sizeof(Params)) == 0 &&
          memcmp(&g.plan, &plan, sizeof(LaunchPlan)) == 0)) {
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
        g = psgpu_ctx::GraphSlot{};
        hipGraph_t graph = nullptr;
        PSGPU_CHECK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        const int rc = launch_all(c, p, plan, s, false);
        const hipError_t ec = hipStreamEndCapture(s, &graph);
        if (rc != PSGPU_RET_SUCCESS) {
            if (graph) (void)hipGraphDestroy(graph);
            reset_run_state(c);
            return rc;
        }
        PSGPU_CHECK(ec);
        const hipError_t ei = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        PSGPU_CHECK(ei);
        g.key = p;
        g.jit = c->jit.kernels.get();
        g.plan = plan;
    }
    PSGPU_CHECK(hipGraphLaunch(g.exec, s));
    return PSGPU_RET_SUCCESS;
}

// Contexts with a run enqueued and not yet collected (psgpu_finish), per device, over the
// process: a run enqueued while no other context has one pending on its device is alone on
// it (a blocking caller, a frame-at-a-time editor, one context queueing its frames) and takes
// the layouts with the shortest spans; runs that overlap other contexts' (contexts taking
// frames in turn) take the layouts with the least total work.
std::atomic<int> g_pendingRuns[64];
constexpr int kMaxWaitingPeers = 4;  // see psgpu_polygonize: crowded
void set_pending(psgpu_ctx* c, bool v) {
    if (c->pending == v) return;
    c->pending = v;
    g_pendingRuns[c->device & 63].fetch_add(v ? 1 : -1);
}

// PrintThreadResults' counters (PS_Polygonizer.cpp:15-18, :443-469): the reference keeps a
// (processed, crossed) pair per TBB worker that ran any MPU, over every Polygonize of the
// process, enumerated in the order the workers first ran one, and cleared by
// PrintThreadResults (.cpp:414-428).  The library's worker is a device context (one stream,
// one polygonization at a time): every finished run adds its range's MPUs and its MPUs with
// at least one triangle to its context's entry; an entry outlives its context, as a TBB
// worker's counter outlives the call that made it, until the next print clears them all.
std::atomic<uint64_t> g_ctxSerial{0};
std::mutex g_threadMu;
std::vector<std::pair<uint64_t, std::pair<uint64_t, uint64_t>>> g_threadCounts;  // serial -> (processed, crossed)
void thread_results_add(uint64_t serial, uint32_t processed, uint32_t crossed) {
    if (processed == 0) return;  // a worker that ran no MPU has no entry (never called local())
    std::lock_guard<std::mutex> lk(g_threadMu);
    for (auto& e : g_threadCounts)
        if (e.first == serial) {
            e.second.first += processed;
            e.second.second += crossed;
            return;
        }
    g_threadCounts.push_back({serial, {processed, crossed}});
}

// Adopt the model's specialised kernels once their compile has finished (wait: block for
// it).  Until then the interpreter runs; its output is bit-identical.  Call with the
// context's device current.
void jit_poll(psgpu_ctx* c, bool wait) {
    JitState& J = c->jit;
    const auto code = J.compile.poll(wait);
    if (!code) return;
    quiesce(c);
    J.kernels = jit_load(**code, c->device, &J.error);
    if (!J.kernels && (*code)->code.size() && J.error.find("dropped") != std::string::npos) {
        // the cached object would not load: compile it afresh (bypassing the disk cache)
        J.compile.start(jit_request(c->model, J.use == 2, false, c->opt.treeSplit != 0));
        if (wait) jit_poll(c, true);
        return;
    }
    if (!J.kernels) fprintf(stderr, "psgpu: JIT unavailable, using the interpreter: %s\n", J.error.c_str());
    J.tier = J.kernels ? (J.use == 2 ? 2 : 1) : 0;
}

// PSGPU_OPT_JIT 3: adopt the baked kernels once their compile has finished (wait: block).
void tier_poll(psgpu_ctx* c, bool wait) {
    JitState& J = c->jit;
    const auto code = J.baked.poll(wait);
    if (!code) return;
    std::string err;
    std::shared_ptr<JitKernels> k = jit_load(**code, c->device, &err);
    if (!k) {  // the structure kernels keep serving this model
        J.tier2Failed = true;
        fprintf(stderr, "psgpu: baked kernels unavailable, the structure kernels stay: %s\n", err.c_str());
        return;
    }
    if (c->pending && c->useGraph) (void)hipStreamSynchronize(c->runStream);  // no graph dies in flight
    drop_graphs(c);  // modules live as long as the process: in-flight runs keep theirs
    J.kernels1 = J.kernels;
    J.kernels = k;
    J.tier = 2;
}

// PSGPU_OPT_JIT 3: count a run of the unchanged model on the structure kernels and start the
// baked compile at the threshold.
void tier_count(psgpu_ctx* c) {
    JitState& J = c->jit;
    if (J.use != 3 || J.tier != 1 || J.baked.pending() || J.tier2Failed) return;
    if (++J.staticRuns < J.tierRuns) return;
    J.baked.start(jit_request(c->model, true, true, c->opt.treeSplit != 0));
}

// Start (or restart) the compile of the current model's kernels.  A compile still running for
// the previous model or options is retired: it ends in the background, before the context goes.
void jit_start(psgpu_ctx* c) {
    JitState& J = c->jit;
    J.kernels.reset();
    J.kernels1.reset();
    J.tier = J.staticRuns = 0;
    J.tier2Failed = false;
    J.compile.drop();
    J.baked.drop();
    if (!J.use || !c->haveModel) return;
    J.compile.start(jit_request(c->model, J.use == 2, true, c->opt.treeSplit != 0));
    jit_poll(c, !J.async);
}

// Put a context whose launch sequence failed part-way back into a usable state: the
// next run's counters and look-back words were to be reset by this run's k_finish.
void reset_run_state(psgpu_ctx* c) {
    const DevCounters init[2] = {empty_counters(), empty_counters()};
    (void)hipStreamSynchronize(c->stream);
    (void)hipMemcpy(c->ctr, init, sizeof(init), hipMemcpyHostToDevice);
    (void)hipMemset(c->scanStatus, 0, 2 * kScanMaxBlocks * sizeof(uint64_t));
    if (c->fqReady) (void)hipMemset(c->fqReady, 0, c->fqReady.cap * sizeof(uint32_t));  // the epochs restart at 0
    (void)hipDeviceSynchronize();
    c->parity = 0;
    c->epochRuns = 0;
    drop_graphs(c);
}

}  // namespace

// ===========================================================================
extern "C" {

const char* psgpu_version(void) { return "parsip_amd 0.1 (gfx950)"; }

void psgpu_tritable(int32_t out[256 * 16]) {
    const CubeTables& T = cube_tables();
    for (int c = 0; c < 256; ++c)
        for (int i = 0; i < 16; ++i) out[c * 16 + i] = T.tri[c][i];
}

uint32_t psgpu_count_mpus(float cellsize, const float lo[3], const float hi[3]) {
    if (!(cellsize > 0.0f)) return 0;
    PsVec3f l{lo[0], lo[1], lo[2]}, h{hi[0], hi[1], hi[2]};
    uint32_t d[3];
    lattice_dims(cellsize, l, h, d);
    return d[0] * d[1] * d[2];
}

int psgpu_mpu_dims(float cellsize, const PsSoaBlobPrims* prims, uint32_t dims[3]) {
    if (!prims || !(cellsize > 0.0f)) return PSGPU_RET_PARAM_ERROR;
    lattice_dims(cellsize, prims->bboxLo, prims->bboxHi, dims);
    return PSGPU_RET_SUCCESS;
}

int psgpu_translate_blobtree_type(int t) { return translate_blobtree_type(t); }

int psgpu_prepare_bboxes(float cellsize, PsSoaBlobPrims* P, PsSoaBoxMatrices* BM, PsSoaBlobOps* O) {
    (void)cellsize;
    return prepare_bboxes(P, BM, O);
}

uint64_t psgpu_debug_device_bytes(void) { return g_deviceBytes.load(); }

int psgpu_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int psgpu_create(int deviceOrdinal, psgpu_ctx** out) {
    if (!out) return PSGPU_RET_PARAM_ERROR;
    *out = nullptr;
    int n = psgpu_device_count();
    if (deviceOrdinal < 0 || deviceOrdinal >= n) return PSGPU_RET_DEVICE_ERROR;
    psgpu_ctx* c = new psgpu_ctx();
    c->device = deviceOrdinal;
    c->serial = ++g_ctxSerial;
    int rc = set_device(c);
    if (rc != PSGPU_RET_SUCCESS) { delete c; return rc; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, deviceOrdinal) == hipSuccess && prop.multiProcessorCount > 0)
        c->numCUs = prop.multiProcessorCount;
    c->opt.splitMaxQueued = 4u * (uint32_t)c->numCUs;
    const CubeTables& T = cube_tables();
    CubeTablesDev tabHost{};
    fill_device_tables(T, tabHost);
    // the set-up copies run on the null stream BEFORE this context's stream exists: a process's
    // first stream created ahead of the null stream's first use shares its hardware queue
    // (tools/queue_probe.py: with 4 engines, the engine on that stream slowed every step ~25%)
    constexpr Growth X = Growth::Exact;
    if (c->dTables.reserve(1, X) != hipSuccess ||
        hipMemcpy(c->dTables, &tabHost, sizeof(CubeTablesDev), hipMemcpyHostToDevice) != hipSuccess ||
        c->dModel.reserve(1, X) != hipSuccess ||
        c->ctr.reserve(2, X) != hipSuccess ||
        c->totals.reserve(16, X) != hipSuccess ||
        c->scanStatus.reserve(2 * kScanMaxBlocks, X) != hipSuccess ||
        hipMemset(c->scanStatus, 0, 2 * kScanMaxBlocks * sizeof(uint64_t)) != hipSuccess ||
        c->hostCtr.reserve(1, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
        hipHostGetDevicePointer(reinterpret_cast<void**>(&c->hostCtrDev), c->hostCtr, 0) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess ||
        c->stream.create(hipStreamNonBlocking) != hipSuccess) {
        psgpu_destroy(c);
        return PSGPU_RET_DEVICE_ERROR;
    }
    *c->hostCtr = empty_counters();
    c->emptyTotals = c->totals + 8;  // {0, 0, 0, 0, 0, 0, no overflow, no error}
    const uint32_t empty[16] = {0, 0, 0, 0, 0, 0, 0x7fffffffu, 0, 0, 0, 0, 0, 0, 0, 0x7fffffffu, 0};
    const DevCounters init[2] = {empty_counters(), empty_counters()};
    if (hipMemcpy(c->totals, empty, sizeof(empty), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(c->ctr, init, sizeof(init), hipMemcpyHostToDevice) != hipSuccess) {
        psgpu_destroy(c);
        return PSGPU_RET_DEVICE_ERROR;
    }
    for (int i = 0; i <= kNumKernels; ++i) (void)c->ev[i].create();
    const char* cullEnv = getenv("PSGPU_CULL");
    if (cullEnv) c->cull = atoi(cullEnv) != 0;
    if (const char* e = getenv("PSGPU_OP_INSIDE")) c->opInside = atoi(e) != 0;
    const char* jitEnv = getenv("PSGPU_JIT");
    if (jitEnv) c->jit.use = std::min(3, std::max(0, atoi(jitEnv)));
    const char* asyncEnv = getenv("PSGPU_JIT_ASYNC");
    if (asyncEnv) c->jit.async = atoi(asyncEnv) != 0;
    if (const char* e = getenv("PSGPU_GRID_FIT")) c->opt.gridFit = atoi(e) != 0;          // 0: persistent grids
    if (const char* e = getenv("PSGPU_FINISH_QUAD")) c->opt.finishQuad = std::min(3, std::max(0, atoi(e)));
    if (const char* e = getenv("PSGPU_VERTEX_WIDE")) c->opt.vertexWide = std::min(2, std::max(0, atoi(e)));
    if (const char* e = getenv("PSGPU_MPU_MARGIN")) c->opt.mpuMarginDiv = std::max(1, atoi(e));
    if (const char* e = getenv("PSGPU_FUSED_SURFACE")) c->opt.fusedSurface = std::min(3, std::max(0, atoi(e)));
    if (const char* e = getenv("PSGPU_FRONT")) c->opt.front = std::min(2, std::max(0, atoi(e)));
    if (const char* e = getenv("PSGPU_SIEVE")) c->opt.sieve = std::min(2, std::max(0, atoi(e)));
    *out = c;
    return PSGPU_RET_SUCCESS;
}

void psgpu_destroy(psgpu_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    set_pending(c, false);
    drop_graphs(c);
    // no compile outlives its context (psgpu_compile.h), and they end ahead of the stream
    c->jit.compile.drain();
    c->jit.baked.drain();
    weld_state_free(c->weld);
    for (Event& e : c->ev) e.reset();
    for (Event& e : c->exportEv) e.reset();
    c->stream.reset();  // ahead of the buffers
    delete c;  // its buffers go with it, on the device made current above
}

int psgpu_set_option(psgpu_ctx* c, int option, int64_t value) {
    if (!c) return PSGPU_RET_PARAM_ERROR;
    const int drc = set_device(c);  // modules load and buffers free on the context's device
    if (drc != PSGPU_RET_SUCCESS) return drc;
    if (option == PSGPU_OPT_KERNEL_TIMING) c->timing = value != 0;
    else if (option == PSGPU_OPT_CULLING) c->cull = value != 0;
    else if (option == PSGPU_OPT_OP_INSIDE) c->opInside = value != 0;
    else if (option == PSGPU_OPT_DEBUG) c->debug = (int)value;
    else if (option == PSGPU_OPT_GRAPH) c->useGraph = value != 0;
    else if (option == PSGPU_OPT_BOUND) c->bound = value != 0;
    else if (option == PSGPU_OPT_CAPACITY && value >= 64 && value <= (1ll << 30)) {
        // restart the output / work-queue buffers at this vertex capacity (they grow on demand);
        // a pending result is dropped with them
        if (c->pending) (void)hipStreamSynchronize(c->runStream);
        set_pending(c, false);
        c->seen = Caps{};
        c->vk.release();
        c->vp.release();
        c->tq.release();
        c->pos.release();
        c->nrm.release();
        c->col.release();
        c->tris.release();
        c->vcap = (uint32_t)value;
        c->tcap = (uint32_t)std::min<int64_t>(2 * value, 0xffffffffll);
        c->vShardCap = (uint32_t)std::max<int64_t>(16, value / kShards);
        c->tShardCap = 2 * c->vShardCap;
        c->haveResult = false;
        ++c->runSeq;
    }
    else if (option == PSGPU_OPT_VERTEX_BLOCKS_PER_CU && value >= 1 && value <= 32) c->opt.vertexBlocksPerCU = (int)value;
    else if (option == PSGPU_OPT_FINISH_BLOCKS_PER_CU && value >= 1 && value <= 32) c->opt.finishBlocksPerCU = (int)value;
    else if (option == PSGPU_OPT_FINISH_QUAD && value >= 0 && value <= 3) c->opt.finishQuad = (int)value;
    else if (option == PSGPU_OPT_VERTEX_WIDE && value >= 0 && value <= 2) c->opt.vertexWide = (int)value;
    else if (option == PSGPU_OPT_TREE_SPLIT && value >= 0 && value <= 2) {
        const bool recompile = value != 0 && c->opt.treeSplit == 0 && c->haveModel && c->splittable &&
                               !(c->jit.kernels && c->jit.kernels->precheckS);
        c->opt.treeSplit = (int)value;
        if (recompile) {  // the loaded kernels lack the split variants: generate them
            quiesce(c);
            jit_start(c);
        }
    }
    else if (option == PSGPU_OPT_SPLIT_MAX_QUEUED && value >= 0 && value <= 0xffffffffll) c->opt.splitMaxQueued = (uint32_t)value;
    else if (option == PSGPU_OPT_FUSED_SURFACE && value >= 0 && value <= 3) c->opt.fusedSurface = (int)value;
    else if (option == PSGPU_OPT_FRONT && value >= 0 && value <= 2) c->opt.front = (int)value;
    else if (option == PSGPU_OPT_SIEVE && value >= 0 && value <= 2) c->opt.sieve = (int)value;
    else if (option == PSGPU_OPT_TIER_RUNS && value >= 1 && value <= (1 << 30)) c->jit.tierRuns = (int)value;
    else if (option == PSGPU_OPT_JIT) {
        if (value < 0 || value > 3) return PSGPU_RET_PARAM_ERROR;
        c->jit.use = (int)value;
        quiesce(c);
        jit_start(c);
    }
    else if (option == PSGPU_OPT_JIT_ASYNC) c->jit.async = value != 0;
    else if (option == PSGPU_OPT_MPU_TICKS) c->mpuTicksOpt = value != 0;  // buffers: next polygonize
    else if (option == PSGPU_OPT_SPANS && value >= 0 && value <= (1 << 20)) {
        // the next `value` runs record their kernel spans, one slot each (then none)
        quiesce(c);
        c->spans.release();
        c->spanCap = c->spanNext = 0;
        if (value > 0) {
            std::vector<uint64_t> init((size_t)value * 2 * kNumStampKernels * kSpanLanes);
            for (size_t i = 0; i < init.size(); i += 2) {
                init[i] = ~0ull;
                init[i + 1] = 0ull;
            }
            PSGPU_CHECK(c->spans.reserve(init.size(), Growth::Exact));
            PSGPU_CHECK(hipMemcpy(c->spans, init.data(), init.size() * 8, hipMemcpyHostToDevice));
            c->spanCap = (uint32_t)value;
        }
    }
    else if (option == PSGPU_OPT_STAMPS && value >= 0 && value <= (1 << 24)) {
        quiesce(c);
        c->stamps.release();
        c->stampCap = 0;
        if (value > 0) {
            const size_t bytes = stamp_bytes((size_t)value);
            PSGPU_CHECK(c->stamps.reserve(bytes / 8, Growth::Exact));  // whole 8-byte words
            PSGPU_CHECK(hipMemset(c->stamps, 0, bytes));  // a kernel a run does not launch leaves no rows
            c->stampCap = (uint32_t)value;
        }
    }
    else return PSGPU_RET_PARAM_ERROR;
    return PSGPU_RET_SUCCESS;
}

int psgpu_set_model(psgpu_ctx* c, const PsSoaBlobPrims* prims, const PsSoaPrimMatrices* mats,
                    const PsSoaBlobOps* ops) {
    if (!c || !prims || !mats || !ops) return PSGPU_RET_PARAM_ERROR;
    int rc = set_device(c);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    DevModel* m = new DevModel;
    rc = build_device_model(*prims, *mats, *ops, *m);
    if (rc != PSGPU_RET_SUCCESS) { delete m; return rc; }
    if (c->pending) (void)hipStreamSynchronize(c->runStream);
    // captured graphs stay valid: specialised modules live as long as the process
    // (jit_get's cache) and the replay key compares the kernels and every parameter.
    // The same model again (build_device_model zeroes every byte first) keeps its kernels,
    // and with PSGPU_OPT_JIT 3 its tier and run count.
    const bool same = c->haveModel && memcmp(&c->model, m, sizeof(DevModel)) == 0;
    c->model = *m;
    delete m;
    c->splittable = jit_splittable(c->model);
    memcpy(&c->primsHost, prims, sizeof(PsSoaBlobPrims));
    if (!same) {  // the same bytes are already in HBM (a blocking caller re-sending its model)
        PSGPU_CHECK(hipMemcpyAsync(c->dModel, &c->model, sizeof(DevModel), hipMemcpyHostToDevice, c->stream));
        PSGPU_CHECK(hipStreamSynchronize(c->stream));
    }
    c->haveModel = true;
    ++c->runSeq;  // a weld belongs to a finished run of the current model
    if (!same || (!c->jit.kernels && !c->jit.compile.pending())) jit_start(c);
    return PSGPU_RET_SUCCESS;
}

int psgpu_polygonize(psgpu_ctx* c, float cellsize, uint32_t mpuBegin, uint32_t mpuEnd, void* stream) {
    if (!c || !c->haveModel) return PSGPU_RET_PARAM_ERROR;
    if (c->primsHost.ctPrims == 0 || !(cellsize > 0.0f)) return PSGPU_RET_PARAM_ERROR;
    int rc = set_device(c);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if (c->pending && c->runStream != s) (void)hipStreamSynchronize(c->runStream);
    // validate into locals first: a rejected call leaves the lattice of a pending run (its
    // finish / export read c->cs and c->dims) untouched
    uint32_t dims[3];
    lattice_dims(cellsize, c->primsHost.bboxLo, c->primsHost.bboxHi, dims);
    const uint64_t total = (uint64_t)dims[0] * dims[1] * dims[2];
    if (total > 0xffffffffull) return PSGPU_RET_PARAM_ERROR;
    const uint32_t end = (uint32_t)std::min<uint64_t>(mpuEnd, total);
    const uint32_t begin = std::min(mpuBegin, end);
    if (end - begin >= kMaxRangeMpus) return PSGPU_RET_PARAM_ERROR;  // TriRec's 20-bit slot field
    c->cs = cellsize;
    memcpy(c->dims, dims, sizeof(dims));
    if (begin != c->mpuBegin || end - begin != c->mpuCount || cellsize != c->lastCs) {
        // another range or lattice: the last run's survivor count says nothing about this
        // one -- size k_mpu for the whole range (no re-run) until a run of it finishes.  A new
        // model on the same lattice (an animation frame) keeps the prediction; a frame that
        // queues more is re-run by finish(), and psgpu_comm_result agrees on that collectively.
        c->last.haveQueued = false;
        c->last.lastV = 0;
    }
    c->lastCs = cellsize;
    c->mpuBegin = begin;
    c->mpuCount = end - begin;
    jit_poll(c, false);
    tier_poll(c, false);
    tier_count(c);
    // capacity from the largest finished run + 1/4 (grows only; finish() still re-runs
    // on an overflow, so a prediction that falls short costs time, never output)
    set_caps(c, grown_ahead(caps_of(c), c->seen));
    const BrickLayout bricks = run_bricks(c);
    rc = ensure_buffers(c, bricks);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    // alone: no OTHER context has a run pending on the device (this context's own earlier
    // runs share its stream, so they never overlap this one)
    const int others = g_pendingRuns[c->device & 63].load() - (c->pending ? 1 : 0);
    c->alone = others == 0;
    // the launches with in-kernel waits (k_surface, k_front) only while at most 3 other contexts
    // of the process have runs in flight on the device: with more, the waiting blocks of all
    // their launches can hold every slot of an XCD that another launch's awaited blocks still
    // need (blocks go to the XCDs round-robin, each XCD dispatching its share in order), and the
    // waits end only at their bounds (6-8 engines on a C4 share: protocol errors, ms per step;
    // profiles/r06_engines_waits.txt)
    c->crowded = others >= kMaxWaitingPeers;
    rc = enqueue(c, s, bricks);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    c->runStream = s;
    set_pending(c, true);
    c->haveResult = false;
    ++c->runSeq;
    return PSGPU_RET_SUCCESS;
}

int psgpu_finish(psgpu_ctx* c, PsMeshInfo* info) {
    if (!c) return PSGPU_RET_PARAM_ERROR;
    if (c->pending) {
        int rc = set_device(c);
        if (rc != PSGPU_RET_SUCCESS) return rc;
        PSGPU_CHECK(hipStreamSynchronize(c->runStream));
        set_pending(c, false);
        // judge it (psgpu_plan.h); grow and re-run while the S2 grid, the work queues or the
        // compact outputs did not fit
        const DevCounters& h = *c->hostCtr;
        const BrickLayout bricks = run_bricks(c);
        bool reran = false;
        RunVerdict verdict;
        for (int attempt = 0;; ++attempt) {
            verdict = judge_run(h, c->run, c->mpuCount, caps_of(c));
            c->last = verdict.last;
            c->seen = caps_max(c->seen, verdict.used);
            if (verdict.fits) break;
            if (attempt == 3) return PSGPU_RET_NOT_ENOUGH_MEM;  // still short after 3 regrowths
            set_caps(c, grown(caps_of(c), verdict));
            rc = ensure_buffers(c, bricks);
            if (rc != PSGPU_RET_SUCCESS) return rc;
            rc = enqueue(c, c->runStream, bricks);
            if (rc != PSGPU_RET_SUCCESS) return rc;
            PSGPU_CHECK(hipStreamSynchronize(c->runStream));
            reran = true;
        }
        if (c->timing && c->mpuCount > 0) {
            for (int k = 0; k < kNumKernels; ++k) {
                float ms = 0.0f;
                if (hipEventElapsedTime(&ms, c->ev[k], c->ev[k + 1]) == hipSuccess) c->lastMs[k] = ms;
            }
        }
        if (verdict.protocol) {
            // an in-kernel wait gave up (an offsets-scan look-back, or k_surface's wait for the
            // scan): the run's offsets are not trusted.  Re-run it once as k_vertex + k_finish,
            // the chain whose kernel boundaries order the scan; a second error fails the call.
            // Known gap (the open high finding): this re-run is checked for a second
            // protocol error only, never judged against the grid and the capacities again.
            fprintf(stderr, "psgpu: device protocol error 0x%x (%s): re-running as separate launches\n",
                    verdict.protocol, c->run.front ? (c->run.surface ? "k_front, k_surface" : "k_front")
                                                   : (c->run.surface ? "k_surface" : "k_vertex"));
            rc = enqueue(c, c->runStream, bricks, true);
            if (rc != PSGPU_RET_SUCCESS) return rc;
            PSGPU_CHECK(hipStreamSynchronize(c->runStream));
            reran = true;
            if (protocol_error(h)) {
                fprintf(stderr, "psgpu: device protocol error 0x%x\n", protocol_error(h));
                return PSGPU_RET_DEVICE_ERROR;
            }
        }
        if (c->debug & (1 << 21)) {  // test hook: this finish fails as a protocol error would (one run)
            c->debug &= ~(1 << 21);
            return PSGPU_RET_DEVICE_ERROR;
        }
        c->info = mesh_info(h, c->run, c->mpuCount, reran);
        c->haveResult = true;
        c->finishedSeq = c->runSeq;
        if (c->countThreads) thread_results_add(c->serial, c->info.ctMPUs, c->info.ctSurfaceMPUs);
    }
    if (!c->haveResult) return PSGPU_RET_PARAM_ERROR;
    if (info) *info = c->info;
    return PSGPU_RET_SUCCESS;
}

int psgpu_download_stamps(psgpu_ctx* c, uint64_t* out, uint32_t* capOut) {
    int rc = finished_run(c);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    if (capOut) *capOut = c->stamps ? c->stampCap : 0u;
    if (!c->stamps || !out) return c->stamps ? PSGPU_RET_SUCCESS : PSGPU_RET_PARAM_ERROR;
    PSGPU_CHECK(hipMemcpy(out, c->stamps, stamp_bytes(c->stampCap), hipMemcpyDeviceToHost));
    return PSGPU_RET_SUCCESS;
}

int psgpu_vertex_queue(psgpu_ctx* c, uint32_t* counts, uint32_t* recs, uint32_t capacity) {
    if (!c || !counts) return PSGPU_RET_PARAM_ERROR;
    int rc = finished_run(c);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    for (int k = 0; k < kShards; ++k) counts[k] = c->mpuCount ? c->hostCtr->shard[k].v : 0u;
    const ShardSums sum(*c->hostCtr);
    if (c->mpuCount && sum.maxV > c->vShardCap) return PSGPU_RET_DEVICE_ERROR;  // finish re-runs until they fit
    if (!recs) return PSGPU_RET_SUCCESS;
    if (c->mpuCount && sum.v > capacity) return PSGPU_RET_PARAM_ERROR;
    std::vector<VertexKey> shard;
    for (int k = 0; k < kShards; ++k) {
        if (counts[k] == 0) continue;
        shard.resize(counts[k]);
        PSGPU_CHECK(hipMemcpy(shard.data(), c->vk + (size_t)k * c->vShardCap, (size_t)counts[k] * sizeof(VertexKey),
                              hipMemcpyDeviceToHost));
        for (const VertexKey& K : shard) {
            *recs++ = K.w;
            *recs++ = K.vidKey & 0xffffu;
        }
    }
    return PSGPU_RET_SUCCESS;
}

int psgpu_mpu_masks(psgpu_ctx* c, uint8_t* queued, uint64_t* masks, uint32_t capacity) {
    if (!c || !queued || !masks) return PSGPU_RET_PARAM_ERROR;
    int rc = finished_run(c);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    if (c->mpuCount > capacity) return PSGPU_RET_PARAM_ERROR;
    if (c->mpuCount == 0) return PSGPU_RET_SUCCESS;
    const size_t n = c->mpuCount;
    PSGPU_CHECK(hipMemcpy(queued, c->passed, n, hipMemcpyDeviceToHost));
    PSGPU_CHECK(hipMemcpy(masks, c->mpuMasks, 4 * n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    for (size_t w = 0; w < n; ++w) {  // passed: 2 = queued for S2 (k_precheck); others have no masks
        queued[w] = queued[w] == 2 ? 1 : 0;
        if (!queued[w] || !c->cull)
            for (int k = 0; k < 4; ++k) masks[4 * w + k] = 0ull;
    }
    return PSGPU_RET_SUCCESS;
}

int psgpu_live_bricks(psgpu_ctx* c, uint32_t* bricks, uint32_t capacity, uint32_t* count) {
    if (!c || !count) return PSGPU_RET_PARAM_ERROR;
    int rc = finished_run(c);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    *count = 0;
    if (c->mpuCount == 0 || !c->run.sieve) return PSGPU_RET_SUCCESS;
    const uint32_t n = c->hostCtr->liveBricks;
    *count = n;
    if (!bricks || n == 0) return PSGPU_RET_SUCCESS;
    if (n > capacity || n > c->liveList.cap) return PSGPU_RET_PARAM_ERROR;
    std::vector<uint64_t> raw(n);
    PSGPU_CHECK(hipMemcpy(raw.data(), c->liveList, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    for (uint32_t k = 0; k < n; ++k) {
        bricks[3 * k] = (uint32_t)raw[k] & 0x1fffffu;
        bricks[3 * k + 1] = (uint32_t)(raw[k] >> 21) & 0x1fffffu;
        bricks[3 * k + 2] = (uint32_t)(raw[k] >> 42);
    }
    return PSGPU_RET_SUCCESS;
}

int psgpu_mpu_octants(psgpu_ctx* c, uint16_t* oct, uint32_t capacity) {
    if (!c || !oct) return PSGPU_RET_PARAM_ERROR;
    int rc = finished_run(c);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    if (c->mpuCount > capacity) return PSGPU_RET_PARAM_ERROR;
    for (uint32_t w = 0; w < c->mpuCount; ++w) oct[w] = 0;
    if (c->mpuCount == 0) return PSGPU_RET_SUCCESS;
    // k_front: 8 sub-queues of fqCap entries; otherwise the kShards queues of pShardCap
    const uint32_t queues = c->run.front ? 8u : (uint32_t)kShards, cap = c->run.front ? c->run.fqCap : c->pShardCap;
    std::vector<uint64_t> q;
    for (uint32_t k = 0; k < queues; ++k) {
        const uint32_t n = c->hostCtr->shard[k].p;
        if (n == 0) continue;
        if (n > cap || (size_t)k * cap + n > c->pq.cap) return PSGPU_RET_DEVICE_ERROR;
        q.resize(n);
        PSGPU_CHECK(hipMemcpy(q.data(), c->pq + (size_t)k * cap, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost));
        for (uint64_t e : q) {
            const uint32_t w = (uint32_t)e - c->mpuBegin;
            if (w >= c->mpuCount) return PSGPU_RET_DEVICE_ERROR;
            oct[w] = (uint16_t)(e >> 32);
        }
    }
    return PSGPU_RET_SUCCESS;
}

int psgpu_s2_passes(psgpu_ctx* c, uint32_t* passes) {
    if (!c || !passes) return PSGPU_RET_PARAM_ERROR;
    int rc = finished_run(c);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    *passes = c->mpuCount ? c->hostCtr->s2Passes : 0u;
    return PSGPU_RET_SUCCESS;
}

int psgpu_download_spans(psgpu_ctx* c, uint64_t* out, uint32_t* runs) {
    if (!c || !runs) return PSGPU_RET_PARAM_ERROR;
    *runs = c->spans ? c->spanNext : 0u;
    if (!c->spans || !out || c->spanNext == 0) return PSGPU_RET_SUCCESS;
    int rc = set_device(c);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    if (c->pending) PSGPU_CHECK(hipStreamSynchronize(c->runStream));
    const size_t per = (size_t)2 * kNumStampKernels * kSpanLanes;
    std::vector<uint64_t> raw((size_t)c->spanNext * per);
    PSGPU_CHECK(hipMemcpy(raw.data(), c->spans, raw.size() * 8, hipMemcpyDeviceToHost));
    for (uint32_t r = 0; r < c->spanNext; ++r)
        for (int k = 0; k < kNumStampKernels; ++k) {
            uint64_t lo = ~0ull, hi = 0ull;
            for (int l = 0; l < kSpanLanes; ++l) {
                const uint64_t* s = &raw[r * per + 2 * ((size_t)k * kSpanLanes + l)];
                lo = std::min(lo, s[0]);
                hi = std::max(hi, s[1]);
            }
            out[(size_t)r * 2 * kNumStampKernels + 2 * k] = lo;
            out[(size_t)r * 2 * kNumStampKernels + 2 * k + 1] = hi;
        }
    return PSGPU_RET_SUCCESS;
}

int psgpu_thread_result_count(void) {
    std::lock_guard<std::mutex> lk(g_threadMu);
    return (int)g_threadCounts.size();
}

int psgpu_print_thread_results(int ctAttempts, uint32_t* lpThreadProcessed, uint32_t* lpThreadCrossed,
                               uint32_t capacity, int print) {
    if (ctAttempts <= 0) return PSGPU_RET_PARAM_ERROR;  // the reference divides by it
    std::lock_guard<std::mutex> lk(g_threadMu);
    const int n = (int)g_threadCounts.size();
    for (int i = 0; i < n; ++i) {
        // the reference's int pair divided by int (.cpp:421-424)
        const uint32_t pr = (uint32_t)(g_threadCounts[i].second.first / (uint64_t)ctAttempts);
        const uint32_t cr = (uint32_t)(g_threadCounts[i].second.second / (uint64_t)ctAttempts);
        if (lpThreadProcessed && (uint32_t)i < capacity) lpThreadProcessed[i] = pr;
        if (lpThreadCrossed && (uint32_t)i < capacity) lpThreadCrossed[i] = cr;
        if (print) printf("Thread#  %d, Processed MPUs %d, Crossed MPUs %d \n", i + 1, (int)pr, (int)cr);
    }
    if (print) fflush(stdout);
    g_threadCounts.clear();
    return n;
}

int psgpu_last_kernel_times(psgpu_ctx* c, float* ms, int maxKernels, const char** names) {
    if (!c) return 0;
    int n = std::min(maxKernels, kNumKernels);
    for (int k = 0; k < n; ++k) {
        if (ms) ms[k] = c->lastMs[k];
        if (names) names[k] = kKernelNames[k];
    }
    return n;
}

int psgpu_mesh_device(psgpu_ctx* c, PsMeshDevice* out) {
    if (!c || !out) return PSGPU_RET_PARAM_ERROR;
    int rc = finished_run(c);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    out->pos = c->pos;
    out->nrm = c->nrm;
    out->col = c->col;
    out->tris = c->tris;
    out->mpuOffsets = c->offs;
    return PSGPU_RET_SUCCESS;
}

int psgpu_download_mesh(psgpu_ctx* c, float* pos, float* nrm, float* col, uint32_t* tris, uint64_t* mpuOffsets) {
    PsMeshInfo I;
    int rc = finished_run(c, &I);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    const size_t V = I.ctVertices, T = I.ctTriangles, N = I.ctMPUs;
    if (pos && V) PSGPU_CHECK(hipMemcpy(pos, c->pos, V * 12, hipMemcpyDeviceToHost));
    if (nrm && V) PSGPU_CHECK(hipMemcpy(nrm, c->nrm, V * 12, hipMemcpyDeviceToHost));
    if (col && V) PSGPU_CHECK(hipMemcpy(col, c->col, V * 12, hipMemcpyDeviceToHost));
    if (tris && T) PSGPU_CHECK(hipMemcpy(tris, c->tris, T * 12, hipMemcpyDeviceToHost));
    if (mpuOffsets) {
        if (N) PSGPU_CHECK(hipMemcpy(mpuOffsets, c->offs, (N + 1) * 8, hipMemcpyDeviceToHost));
        else mpuOffsets[0] = 0;
    }
    return PSGPU_RET_SUCCESS;
}

namespace {
// S1 survivors of the last run (global ids, ascending), from the per-MPU flags.
int survivors(psgpu_ctx* c, std::vector<uint32_t>& ids) {
    ids.clear();
    if (!c->mpuCount) return PSGPU_RET_SUCCESS;
    std::vector<uint8_t> passed(c->mpuCount);
    PSGPU_CHECK(hipMemcpy(passed.data(), c->passed, passed.size(), hipMemcpyDeviceToHost));
    for (uint32_t l = 0; l < c->mpuCount; ++l)
        if (passed[l]) ids.push_back(c->mpuBegin + l);
    return PSGPU_RET_SUCCESS;
}
}  // namespace

int psgpu_download_stats(psgpu_ctx* c, PsMpuStats* stats) {
    PsMeshInfo I;
    int rc = finished_run(c, &I);
    if (rc != PSGPU_RET_SUCCESS || !stats) return rc == PSGPU_RET_SUCCESS ? PSGPU_RET_PARAM_ERROR : rc;
    std::vector<uint32_t> ids;
    rc = survivors(c, ids);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    std::vector<uint64_t> cnt(c->mpuCount);
    if (c->mpuCount) PSGPU_CHECK(hipMemcpy(cnt.data(), c->counts, (size_t)c->mpuCount * 8, hipMemcpyDeviceToHost));
    memset(stats, 0, sizeof(PsMpuStats) * c->mpuCount);
    for (uint32_t m : ids) {
        PsMpuStats& s = stats[m - c->mpuBegin];
        s.passedPrecheck = 1;
        s.ctFieldEvals = 128;
    }
    for (uint32_t l = 0; l < c->mpuCount; ++l) {
        stats[l].ctVertices = (uint32_t)cnt[l];
        stats[l].ctTriangles = (uint32_t)(cnt[l] >> 32);
    }
    return PSGPU_RET_SUCCESS;
}
// MPUSTATS (PS_Polygonizer.h:201-207, written at .cpp:449-461): the per-MPU device ticks of
// the last run on the host's CLOCK_REALTIME nanosecond scale (legacy TBB's tick_count on
// Linux).  The device clock (s_memrealtime, wall-clock rate from the runtime) is mapped by
// bracketing one reading of it (k_clock_probe, stored straight into mapped host memory)
// between two host readings; of 8 tries the tightest bracket gives the offset, which is then
// good to half its width (a few microseconds; MPU ticks are tens of microseconds apart).
int psgpu_download_process_stats(psgpu_ctx* c, PsMpuProcessStats* out) {
    int rc = finished_run(c);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    if (!out || !c->runTicks) return PSGPU_RET_PARAM_ERROR;
    const uint32_t n = c->mpuCount;
    if (!n) return PSGPU_RET_SUCCESS;
    std::vector<uint64_t> t((size_t)n * 4);
    PSGPU_CHECK(hipMemcpy(t.data(), c->mpuTicks, t.size() * 8, hipMemcpyDeviceToHost));
    int khz = 0;
    PSGPU_CHECK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device));
    if (khz <= 0) return PSGPU_RET_DEVICE_ERROR;
    PSGPU_CHECK(c->clockProbe.reserve(8, hipHostMallocMapped | hipHostMallocCoherent));
    uint64_t* const probe = c->clockProbe;
    uint64_t* dProbe = nullptr;
    PSGPU_CHECK(hipHostGetDevicePointer(reinterpret_cast<void**>(&dProbe), probe, 0));
    auto host_ns = [] {
        timespec ts;
        clock_gettime(CLOCK_REALTIME, &ts);
        return (int64_t)ts.tv_sec * 1000000000ll + (int64_t)ts.tv_nsec;
    };
    int64_t bestWidth = INT64_MAX, hostMid = 0;
    uint64_t devAt = 0;
    for (int k = 0; k < 8; ++k) {
        __atomic_store_n(probe, 0ull, __ATOMIC_RELEASE);
        const int64_t h0 = host_ns();
        PSGPU_CHECK(launch_clock_probe(dProbe, c->stream));
        uint64_t d = 0;
        for (uint64_t spin = 0; (d = __atomic_load_n(probe, __ATOMIC_ACQUIRE)) == 0ull; ++spin)
            if ((spin & 1023) == 1023 && hipStreamQuery(c->stream) != hipErrorNotReady) {
                d = __atomic_load_n(probe, __ATOMIC_ACQUIRE);
                if (d == 0ull) return PSGPU_RET_DEVICE_ERROR;  // finished (or failed) without a reading
                break;
            }
        const int64_t h1 = host_ns();
        if (h1 - h0 < bestWidth) {
            bestWidth = h1 - h0;
            hostMid = h0 + (h1 - h0) / 2;
            devAt = d;
        }
    }
    PSGPU_CHECK(hipStreamSynchronize(c->stream));
    const double nsPerTick = 1.0e6 / (double)khz;
    auto to_ns = [&](uint64_t tick) { return hostMid + (int64_t)llround((double)((int64_t)(tick - devAt)) * nsPerTick); };
    for (uint32_t l = 0; l < n; ++l) {
        const uint64_t* r = &t[(size_t)4 * l];
        const bool s2 = r[2] != 0ull;
        out[l].threadID = s2 ? (r[3] >> 32) : (r[3] & 0xffffffffull);
        out[l].tickStart = to_ns(r[0]);
        out[l].tickEnd = to_ns(s2 ? r[2] : r[1]);
    }
    return PSGPU_RET_SUCCESS;
}

// Per-MPU work of the last run in lane-evaluations: 8 (S1) + 64 (field
// bounds of a survivor) or 512 (S2 cache of a queued survivor) + 8 per vertex (4 root
// samples, value and 3 normal samples).  Balances MPU ranges across devices.
int psgpu_mpu_costs(psgpu_ctx* c, uint32_t* costs) {
    PsMeshInfo I;
    int rc = finished_run(c, &I);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    if (!costs) return PSGPU_RET_PARAM_ERROR;
    const uint32_t n = c->mpuCount;
    if (!n) return PSGPU_RET_SUCCESS;
    std::vector<uint8_t> passed(n);
    std::vector<uint64_t> cnt(n);
    PSGPU_CHECK(hipMemcpy(passed.data(), c->passed, n, hipMemcpyDeviceToHost));
    PSGPU_CHECK(hipMemcpy(cnt.data(), c->counts, (size_t)n * 8, hipMemcpyDeviceToHost));
    for (uint32_t l = 0; l < n; ++l)
        costs[l] = 8u + (passed[l] == 1 ? 64u : 0u) + (passed[l] == 2 ? 512u : 0u) + 8u * (uint32_t)cnt[l];
    return PSGPU_RET_SUCCESS;
}

int psgpu_split_costs(const uint32_t* costs, uint32_t n, uint32_t parts, uint32_t begin, uint32_t* bounds) {
    return split_costs(costs, n, parts, begin, bounds);
}

int psgpu_polygonize_mpus(psgpu_ctx* c, float cellsize, const PsSoaBlobPrims* prims, const PsSoaPrimMatrices* mats,
                          const PsSoaBlobOps* ops, PsMPU* mpus, uint32_t capacity, uint32_t* outCt,
                          PsMpuStats* stats) {
    if (!c || !prims) return PSGPU_RET_PARAM_ERROR;
    if (prims->ctPrims == 0) return PSGPU_RET_PARAM_ERROR;  // Polygonize :322-323
    const int64_t tCall = now_ns();
    int rc = psgpu_set_model(c, prims, mats, ops);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    rc = psgpu_polygonize(c, cellsize, 0, 0xffffffffu, nullptr);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    if (!mpus) {  // the reference's own errors first (count, overflow), then the null
        rc = psgpu_export_polympus(c, nullptr, capacity, outCt);
        return rc;
    }
    return export_blocking(c, mpus, capacity, outCt, stats, tCall);
}

int psgpu_polygonize_mpus_ex(psgpu_ctx* c, float cellsize, const PsSoaBlobPrims* prims, const PsSoaPrimMatrices* mats,
                             const PsSoaBlobOps* ops, PsMPU* mpus, uint32_t capacity, uint32_t* outCt,
                             PsMpuStats* stats, PsMpuProcessStats* processStats) {
    if (!c) return PSGPU_RET_PARAM_ERROR;
    if (!processStats) return psgpu_polygonize_mpus(c, cellsize, prims, mats, ops, mpus, capacity, outCt, stats);
    const int was = c->mpuTicksOpt;
    c->mpuTicksOpt = 1;  // this call's run records the ticks (Polygonize :379 hands lpProcessStats on)
    int rc = psgpu_polygonize_mpus(c, cellsize, prims, mats, ops, mpus, capacity, outCt, stats);
    c->mpuTicksOpt = was;
    // ctMPUs entries, as PolyMPUs: only on success (on -4 the caller's array may be shorter)
    if (rc == PSGPU_RET_SUCCESS) rc = psgpu_download_process_stats(c, processStats);
    return rc;
}

// Field probe (FieldComputer::fieldValue / fieldValueAndColor on arbitrary points).
// mode 0: 4-lane groups (consecutive points), 1: per point, 2: per point + colour.
int psgpu_field_values(psgpu_ctx* c, const float* xyz, uint32_t n, int mode, float* out, float* colOut) {
    if (!c || !c->haveModel || !xyz || !out || mode < 0 || mode > 2) return PSGPU_RET_PARAM_ERROR;
    int rc = set_device(c);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    jit_poll(c, false);
    if (n == 0) return PSGPU_RET_SUCCESS;
    DevBuf<float> bx, bout, bcol;  // freed on every return
    PSGPU_CHECK(bx.reserve((size_t)n * 3, Growth::Exact));
    PSGPU_CHECK(bout.reserve((size_t)n, Growth::Exact));
    PSGPU_CHECK(bcol.reserve((size_t)n * 3, Growth::Exact));
    float *dx = bx, *dout = bout, *dcol = bcol;
    PSGPU_CHECK(hipMemcpy(dx, xyz, (size_t)n * 12, hipMemcpyHostToDevice));
    const BrickLayout bricks = run_bricks(c);
    Params p = make_params(c, bricks, plan_run(c, bricks, false));
    hipError_t e;
    if (c->jit.kernels) {
        void* args[] = {&p, &dx, &dout, &dcol, &n, &mode};
        e = hipModuleLaunchKernel(c->jit.kernels->probe, (n + 255) / 256, 1, 1, 256, 1, 1, 0, c->stream, args, nullptr);
    } else {
        e = launch_probe(p, c->stream, dx, dout, dcol, n, mode);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(out, dout, (size_t)n * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && colOut) e = hipMemcpy(colOut, dcol, (size_t)n * 12, hipMemcpyDeviceToHost);
    return hip_fail(e, "psgpu_field_values");
}

// Host-only: build the device image of a model and compile its specialised kernels
// (no GPU needed).  Returns the code-object size, or a negative error code.
long psgpu_jit_compile(const PsSoaBlobPrims* prims, const PsSoaPrimMatrices* mats, const PsSoaBlobOps* ops,
                       int mode, char* log, size_t cap) {
    if (!prims || !mats || !ops) return PSGPU_RET_PARAM_ERROR;
    std::unique_ptr<DevModel> m(new DevModel);
    int rc = build_device_model(*prims, *mats, *ops, *m);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    std::string err;
    long n = jit_compile_only(*m, (mode & 3) == 2, &err, (mode & 4) != 0);
    if (log && cap) {
        const size_t k = std::min(cap - 1, err.size());
        memcpy(log, err.data(), k);
        log[k] = 0;
    }
    return n < 0 ? PSGPU_RET_DEVICE_ERROR : n;
}

// Host-only: the device image of a model (DevModel, psgpu_model.h) as the kernels read it.
long psgpu_model_image(const PsSoaBlobPrims* prims, const PsSoaPrimMatrices* mats, const PsSoaBlobOps* ops,
                       void* out, size_t cap) {
    if (!prims || !mats || !ops) return PSGPU_RET_PARAM_ERROR;
    std::unique_ptr<DevModel> m(new DevModel);
    const int rc = build_device_model(*prims, *mats, *ops, *m);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    if (out && cap >= sizeof(DevModel)) memcpy(out, m.get(), sizeof(DevModel));
    return (long)sizeof(DevModel);
}

// The context's JIT state once whatever has finished compiling is adopted (wait: block for it).
static JitState& jit_now(psgpu_ctx* c, bool wait) {
    if ((c->jit.compile.pending() || c->jit.baked.pending()) && set_device(c) == PSGPU_RET_SUCCESS) {
        jit_poll(c, wait);
        tier_poll(c, wait);
    }
    return c->jit;
}
// Whether the current model runs on run-time specialised kernels (1) or the interpreter (0).
int psgpu_jit_active(psgpu_ctx* c) { return c && jit_now(c, false).kernels ? 1 : 0; }
int psgpu_jit_pending(psgpu_ctx* c) { return c && jit_now(c, false).compile.pending() ? 1 : 0; }
int psgpu_jit_wait(psgpu_ctx* c) { return c && jit_now(c, true).kernels ? 1 : 0; }
int psgpu_jit_tier(psgpu_ctx* c) { return c ? jit_now(c, false).tier : 0; }

// Generated specialised source for the current model (NUL-terminated, truncated to cap).
int psgpu_jit_source(psgpu_ctx* c, char* buf, size_t cap) {
    if (!c || !c->haveModel) return PSGPU_RET_PARAM_ERROR;
    const std::string s = jit_source(c->model, c->jit.tier == 2 || c->jit.use == 2, c->opt.treeSplit != 0);
    if (buf && cap) {
        const size_t n = std::min(cap - 1, s.size());
        memcpy(buf, s.data(), n);
        buf[n] = 0;
    }
    return (int)s.size();
}

}  // extern "C"
