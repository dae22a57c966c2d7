// psgpu_internal.h — the device context shared by the library's host sources
// (psgpu_host.cpp: one context, psgpu_export.cpp: its blocking export, psgpu_group.cpp: contexts
// over several devices, psgpu_comm.cpp: the multi-process count exchange).  Not part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <memory>
#include <string>
#include <vector>

#include "../../include/parsip_gpu.h"
#include "psgpu_buf.h"
#include "psgpu_jit.h"
#include "psgpu_model.h"
#include "psgpu_phase_times.h"
#include "psgpu_plan.h"
#include "psgpu_pool.h"

namespace psgpu {
constexpr int kNumKernels = 4;
constexpr int kExportPieces = 16;  // at most, in the blocking export (psgpu_export.cpp export_stage)
constexpr size_t kExportPieceBytes = 1u << 20;  // its target piece size

// The device weld of a finished run (psgpu_weld.hip): its own buffers, allocated on the first
// psgpu_weld of the context, grown on demand, freed by psgpu_destroy (weld_free).  A group
// keeps one of its own for psgpu_group_weld, on the gathering part's device (psgpu_group.cpp).
constexpr int kWeldPhases = 6;  // psgpu_weld_times: the whole weld, then its five launches

// The shells of a welded mesh (psgpu_shells.hip): topology, area and volume of its connected
// components.  Part of the weld it describes, so a context's weld and a group's both have one;
// its buffers come with the first psgpu_weld_shells, grow on demand and go with the weld's.
constexpr int kShellsPhases = 11;  // psgpu_weld_shells_times: the whole call, then its ten steps
struct ShellsState {
    DevBuf<unsigned char> table;   // open-addressing edge table: keys (8 B a slot), then use counts (8 B a slot)
    DevBuf<uint32_t> parent;       // per welded vertex: union-find parent, then the shell index of a root
    DevBuf<uint32_t> vertexShell;  // per welded vertex: its root, then its shell index
    DevBuf<uint32_t> triShell;     // per triangle
    DevBuf<uint64_t> blockCnt;     // per block of vertices: roots, scanned
    DevBuf<unsigned char> ctl;     // error word, largest |coordinate|, the mesh totals
    DevBuf<unsigned char> acc;     // per shell: counts, bounding box keys, the four integer sums
    DevBuf<PsShell> shells;
    bool valid = false;              // holds the shells of the weld beside it (a new weld clears it)
    PsShellsInfo info{};
    PhaseTimes<kShellsPhases> times;
};

// The welded mesh filtered by shell (psgpu_filter.hip): the stable compaction of the shells
// that pass psgpu_weld_filter's criteria.  Part of the weld and the shells result it was made
// from; its buffers come with the first psgpu_weld_filter, grow on demand and go with the weld's.
constexpr int kFilterPhases = 7;  // psgpu_weld_filter_times: the whole call, then its six steps
struct FilterState {
    DevBuf<uint8_t> mask;        // per shell: the caller's mask, uploaded
    DevBuf<uint8_t> keep;        // per shell: it stays
    DevBuf<uint64_t> shellCnt;   // per block of shells: kept, scanned
    DevBuf<uint64_t> blockCnt;   // per block of vertices and triangles: kept | kept << 32, scanned
    DevBuf<uint32_t> ctl;        // error word, then the kept shells, vertices and triangles
    DevBuf<float> pos;           // the filtered mesh
    DevBuf<float> nrm;
    DevBuf<float> col;
    DevBuf<uint32_t> tris;
    DevBuf<uint32_t> vertexMap;  // per welded vertex
    DevBuf<uint32_t> shellMap;   // per shell
    DevBuf<PsShell> shells;      // the kept shells' records
    bool valid = false;          // holds a filter of the shells beside it (a new weld or shells call clears it)
    PsFilterInfo info{};
    PhaseTimes<kFilterPhases> times;
};

struct WeldState {
    DevBuf<unsigned char> table;  // open-addressing table: edge ids (8 B a slot), then minima (4 B a slot)
    DevBuf<uint32_t> rep;         // per input vertex: its representative (the smallest index on its edge)
    DevBuf<uint32_t> kid;         // per kept input vertex: its welded id
    DevBuf<uint32_t> map;         // vertexMap
    DevBuf<uint64_t> blockCnt;    // per block of vertices: kept | seam << 32, scanned
    DevBuf<float> pos;            // the welded mesh
    DevBuf<float> nrm;
    DevBuf<float> col;
    DevBuf<uint32_t> tris;
    uint32_t colW = 3;               // floats a colour: 3 (rgb), or 4 for the compat context's rgba (psgpu_gui.hip);
                                     // the filter's colours beside it have the same width
    uint64_t doneSeq = ~0ull;        // psgpu_ctx::runSeq of the run the buffers hold the weld of
    PsWeldInfo info{};
    PhaseTimes<kWeldPhases> times;    // a context's weld (a group times its own phases)
    ShellsState shells;               // psgpu_weld_shells of this weld
    FilterState filter;               // psgpu_weld_filter of this weld and those shells
};

}  // namespace psgpu

struct psgpu_ctx {
    using JitKernels = psgpu::JitKernels;
    using DevModel = psgpu::DevModel;
    using Params = psgpu::Params;
    using DevCounters = psgpu::DevCounters;
    using VertexKey = psgpu::VertexKey;
    using VertexPos = psgpu::VertexPos;
    using TriRec = psgpu::TriRec;
    using CubeTablesDev = psgpu::CubeTablesDev;
    static constexpr int kNumKernels = psgpu::kNumKernels;
    int device = 0;
    uint64_t serial = 0;  // process-unique id: this context's PrintThreadResults entry
    bool countThreads = true;  // finished runs add to that entry (off for a group's planning runs)
    int numCUs = 256;
    psgpu::Stream stream;
    PsSoaBlobPrims primsHost;  // bbox + counts of the current model
    DevModel model{};
    psgpu::DevBuf<DevModel> dModel;
    psgpu::DevBuf<CubeTablesDev> dTables;
    psgpu::JitState jit;  // the model's run-time kernels, their tier and their compiles (psgpu_jit.h)
    // this run enqueued while no other run of the process was pending on the device (a
    // blocking caller): the layout defaults pick the shorter-span (latency) layouts
    bool alone = false;
    // ... or while 4 or more other contexts have runs pending on it: no in-kernel waits then
    bool crowded = false;
    bool haveModel = false;
    int cull = 1;
    int debug = 0;
    psgpu::LaunchOptions opt;  // what plan_launch (psgpu_plan.h) shapes a run by: the launch options,
    psgpu::LastRun last;       // ... and the last finished run's counts
    psgpu::LaunchPlan run{};   // the launch shape of the last enqueued run
    bool splittable = false;  // the model's walk splits at the root (jit_splittable)
    psgpu::DevBuf<uint32_t> fqReady;  // k_front: per queue entry, the tag of the run that published it
    int timing = 0;
    // geometry of the last run
    float cs = 0.0f;
    uint32_t dims[3] = {0, 0, 0};
    uint32_t mpuBegin = 0, mpuCount = 0;
    hipStream_t runStream = nullptr;  // borrowed: the caller's, or `stream`
    bool pending = false;
    bool haveResult = false;
    // device buffers
    psgpu::DevBuf<uint64_t> pq;         // sharded S1 survivor queues (id | octant verdicts << 32)
    psgpu::DevBuf<uint64_t> pqMask;     // 4 words per queue entry (culling and op-inside mask of the MPU box)
    psgpu::DevBuf<uint64_t> liveList;   // k_sieve's list of live bricks (one word per brick of the range)
    uint32_t pShardCap = 0;
    float lastCs = 0.0f;            // the cell size of the last enqueued run
    psgpu::DevBuf<uint64_t> scanStatus; // 2 x kScanMaxBlocks look-back words (alternating runs)
    uint32_t parity = 0;            // which counter / status set the next run uses
    // runs launched since the counter sets last started at epoch 0 = the next run's epoch
    // (DevCounters::epoch; k_front tags its queue entries epoch + 1, which must never wrap to 0)
    uint64_t epochRuns = 0;
    psgpu::DevBuf<uint64_t> counts;
    psgpu::DevBuf<uint8_t> passed;      // per MPU: passed S1
    int bound = 1;                  // prove S1 survivors empty by field bounds in k_precheck
    psgpu::DevBuf<uint64_t> mpuMasks;   // 4 words per MPU of the range (the same two masks, box + delta)
    bool opInside = true;           // PSGPU_OPT_OP_INSIDE: k_precheck makes op-inside masks
    psgpu::DevBuf<uint64_t> offs;
    psgpu::DevBuf<VertexKey> vk;
    psgpu::DevBuf<VertexPos> vp;
    psgpu::DevBuf<TriRec> tq;
    psgpu::DevBuf<float> pos;
    psgpu::DevBuf<float> nrm;
    psgpu::DevBuf<float> col;
    psgpu::DevBuf<uint32_t> tris;
    psgpu::DevBuf<DevCounters> ctr;     // two sets, alternating runs
    psgpu::DevBuf<uint32_t> totals;     // 8 words of the last run's totals (k_finish), for RCCL,
    uint32_t* emptyTotals = nullptr;    // then 8 words of an empty run's (totals + 8)
    psgpu::DevBuf<uint64_t> stamps;     // per-wave timeline (PSGPU_OPT_STAMPS), 4 x stampCap x 3 words
    uint32_t stampCap = 0;
    psgpu::DevBuf<uint64_t> spans;      // per-run kernel spans (PSGPU_OPT_SPANS): spanCap x 4 x 2 words
    uint32_t spanCap = 0, spanNext = 0;
    int mpuTicksOpt = 0;                // PSGPU_OPT_MPU_TICKS: runs record per-MPU ticks (MPUSTATS)
    psgpu::DevBuf<uint64_t> mpuTicks;   // 4 words per MPU of the range (Params::mpuTicks)
    bool runTicks = false;              // the last enqueued run recorded them
    psgpu::PinnedBuf<uint64_t> clockProbe;  // pinned, mapped: one device clock reading (k_clock_probe)
    psgpu::PinnedBuf<DevCounters> hostCtr;  // pinned, mapped: written by k_finish
    DevCounters* hostCtrDev = nullptr;  // its device address
    psgpu::PinnedBuf<unsigned char> hostStage;  // pinned staging for the blocking PolyMPUs export
    psgpu::Event exportEv[2];            // the export's metadata, then its packing kernel
    uint32_t exportEpoch = 0;            // the blocking export's flag value (k_export_pack), never 0
    std::unique_ptr<psgpu::ScatterPool> scatterPool;  // the export's scatter threads, made on first use
    uint32_t vcap = 1u << 20, tcap = 1u << 21;               // compact mesh capacity
    uint32_t vShardCap = 1u << 15, tShardCap = 1u << 16;      // work-queue capacity per shard
    psgpu::Event ev[kNumKernels + 1];
    int useGraph = 0;  // replay repeated launch sequences from a hipGraph (measured slower on ROCm 7.2)
    struct GraphSlot {
        hipGraphExec_t exec = nullptr;
        JitKernels* jit = nullptr;
        Params key{};
        psgpu::LaunchPlan plan{};
    } graphs[2];
    float lastMs[kNumKernels] = {};
    PsMeshInfo info{};
    // high-water marks of finished runs: the next run's buffers are sized from them
    // (an animation whose mesh grows frame to frame does not pay a synchronous re-run)
    psgpu::Caps seen{};
    // psgpu_weld: runSeq counts whatever supersedes a result (set_model, polygonize, a
    // capacity restart), finishedSeq is its value when psgpu_finish last collected a run
    uint64_t runSeq = 0, finishedSeq = ~0ull;
    psgpu::WeldState weld;
};

namespace psgpu {
// HIP error -> library return code (prints the failing call).
int hip_fail(hipError_t e, const char* what);
// Make the context's device current on the calling thread.
int set_device(psgpu_ctx* c);
// The one way to a collected run, for every entry point that reads a finished run's buffers:
// psgpu_finish (which makes the device current only while a run is pending), then set_device --
// the calling thread may have used another device since.  PARAM_ERROR for a null context.
int finished_run(psgpu_ctx* c, PsMeshInfo* info = nullptr);
// Free a weld's buffers and events (psgpu_weld.hip), a context's or a group's; its device is current.
void weld_state_free(WeldState& W);
// The context's run is finished, superseded by nothing newer, and whole: it can be welded;
// ctx_welded: ... and c->weld holds its weld.
bool weld_run_ready(const psgpu_ctx* c);
inline bool ctx_welded(const psgpu_ctx* c) { return weld_run_ready(c) && c->weld.doneSeq == c->runSeq; }
// The lattice's edge ids fit their 20 bits a coordinate.
bool weld_lattice_fits(const uint32_t* dims);
// The edge id of every vertex of the context's finished run (all ones: not on an MPU face) into
// edge[0 .. ctVertices) on the context's device, enqueued on s; the context's device is current.
int weld_edges(psgpu_ctx* c, uint64_t* edge, hipStream_t s);
// One weld in three steps (its device current): a context's (psgpu_weld: `records`' vertex records
// name the edges) or a group's (psgpu_group_weld: the gathered mesh, its edge ids in edge[0 .. V)).
struct WeldInput {
    const float *pos, *nrm, *col;  // col: W.colW floats a vertex
    const uint32_t* tris;
    uint32_t V, T;
    const uint64_t* edge;
    const psgpu_ctx* records;
};
// W reset (no weld, shells, filter or times) for a mesh of V vertices and T triangles.  False:
// the mesh is empty, W holds its weld of run `seq` (*info filled) and there is nothing to launch.
bool weld_begin(WeldState& W, uint32_t V, uint32_t T, uint64_t seq, PsWeldInfo* info);
// W's buffers grown, then on s six marks: before the table fill, after the mark kernel
// (k_weld_mark or k_weld_mark_ids), after resolve, scan, emit and map.
int weld_enqueue(WeldState& W, const WeldInput& in, hipStream_t s, PhaseCursor marks);
// Waits for s: W holds the weld of run `seq` (*info filled).
int weld_end(WeldState& W, hipStream_t s, uint64_t seq, PsWeldInfo* info);
// What psgpu_weld_device / psgpu_download_weld and the group's twins hand out of a finished weld
// (the callers check that W holds one; for the download its device is current).
int weld_device(const WeldState& W, PsWeldDevice* out);
int weld_download(const WeldState& W, float* pos, float* nrm, float* col, uint32_t* tris, uint32_t* vertexMap);
int weld_times(const WeldState& W, float* ms, int maxPhases, const char** names);
// k_weld_scan on its own: blockCnt[0 .. blocks) becomes its exclusive scan, blockCnt[blocks] the
// total (both 32-bit halves of a word are scanned), enqueued on s.
void weld_scan_blocks(uint64_t* blockCnt, uint32_t blocks, hipStream_t s);
// The shells of a weld (psgpu_shells.hip), for a context's weld and a group's alike; the weld's
// device is current.  shells_run: W holds a finished weld (W.info); blocking on s; `timed`
// records W.shells.times.  The others serve W.shells once shells_run has succeeded
// (W.shells.valid).
int shells_run(WeldState& W, hipStream_t s, bool timed, PsShellsInfo* info);
int shells_device(const WeldState& W, PsShellsDevice* out);
int shells_download(const WeldState& W, PsShell* shells, uint32_t capacity, uint32_t* vertexShell, uint32_t* triShell);
int shells_times(const WeldState& W, float* ms, int maxPhases, const char** names);
// The filter of a weld by its shells (psgpu_filter.hip), for a context's weld and a group's
// alike; the weld's device is current.  filter_run: W holds a finished weld; PARAM_ERROR unless
// W.shells.valid; blocking on s; `timed` records W.filter.times.  The others serve W.filter once
// filter_run has succeeded on the current shells (W.filter.valid).
int filter_run(WeldState& W, hipStream_t s, bool timed, const PsShellFilter* f, const uint8_t* mask, uint32_t maskCount,
               PsFilterInfo* info);
int filter_device(const WeldState& W, PsFilterDevice* out);
int filter_download(const WeldState& W, float* pos, float* nrm, float* col, uint32_t* tris, uint32_t* vertexMap,
                    uint32_t* shellMap, PsShell* shells, uint32_t shellCapacity);
int filter_times(const WeldState& W, float* ms, int maxPhases, const char** names);
// The blocking export of a finished run in two steps (psgpu_export.cpp): enqueue the copies of
// the compact mesh (mesh), the S1 flags and (stats) the per-MPU counts into the context's
// pinned staging buffer, then wait and scatter into PolyMPUs / PsMpuStats.
struct ExportStage {
    bool mesh = false, stats = false;
    size_t V = 0, T = 0, N = 0;
    size_t oOffs = 0, oPos = 0, oNrm = 0, oCol = 0, oTris = 0, oPass = 0, oCnt = 0;
    // the mesh, packed as `pieces` MPU ranges (pos | nrm | col | 16-bit triangle corners of
    // each, psgpu_launch.h PackSrc) at oMesh, piece k complete when its packBlocks flags at
    // oFlags + 4 k packBlocks equal epoch: the scatter of one piece overlaps the
    // transfer of the next.  oFlags = 0 in every call: the flag words hold nothing else
    int pieces = 0;
    size_t oMesh = 0, meshBytes = 0, oFlags = 0;
    uint32_t epoch = 0, packBlocks = 0;
};
// `after`: an event the packing kernel waits for (the previous part's packing on the same
// device, so the parts' pieces cross the link in range order)
int export_stage(psgpu_ctx* c, bool mesh, bool stats, ExportStage* st, hipEvent_t after = nullptr);
int export_scatter(psgpu_ctx* c, const ExportStage& st, PsMPU* mpus, PsMpuStats* stats, const int64_t* trace = nullptr);
bool export_trace_on();
inline int64_t now_ns() {
    return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
// One staged export's scatter into PolyMPUs, split so that a group's parts go in one pass of
// the thread pool (scatter_jobs): prepare (after the metadata), task per thread, finish.
struct ScatterJob {
    psgpu_ctx* c = nullptr;
    const ExportStage* S = nullptr;
    PsMPU* mpus = nullptr;
    const uint64_t* off = nullptr;
    const uint8_t* passed = nullptr;
    const unsigned char* mesh = nullptr;
    const uint32_t* flags = nullptr;
    float side = 0.0f;
    bool active = false;
    std::atomic<bool> failed{false};
    uint32_t pm[kExportPieces + 1] = {};
    size_t pbase[kExportPieces] = {}, pv0[kExportPieces] = {}, pt0[kExportPieces] = {}, pnv[kExportPieces] = {};
    int prepare(psgpu_ctx* c, const ExportStage& st, PsMPU* mpus);
    std::atomic<int> ready{0};        // pieces known to be in (-1: the packing kernel failed)
    // PSGPU_EXPORT_TRACE: steady-clock ns when the first scatter task started, when each piece
    // was seen in (export_blocking prints the call's phases to stderr)
    bool trace = false;
    std::atomic<int64_t> tFirstTask{0};
    int64_t tPiece[kExportPieces] = {};
    std::atomic<bool> polling{false};  // a thread is reading the flags
    uint32_t pollBlock = 0;            // the poller's place in the current piece's flags (under `polling`)
    bool wait_piece(int k);
    bool range(uint32_t lb, uint32_t le, int* have);
    void task(unsigned k, unsigned nth);
    int finish(PsMpuStats* stats);
};
int scatter_jobs(psgpu_ctx* c, ScatterJob* jobs, size_t n);
// One context's blocking export, run collected first (psgpu_export_polympus, psgpu_polygonize_mpus).
// tCall: when the caller's call began, for PSGPU_EXPORT_TRACE (0: now).
int export_blocking(psgpu_ctx* c, PsMPU* mpus, uint32_t capacity, uint32_t* outCt, PsMpuStats* stats, int64_t tCall = 0);
}  // namespace psgpu

#define PSGPU_CHECK(expr)                                           \
    do {                                                            \
        hipError_t _e = (expr);                                     \
        if (_e != hipSuccess) return psgpu::hip_fail(_e, #expr);    \
    } while (0)
