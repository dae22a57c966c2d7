// psgpu_export.cpp — the blocking export of a finished run (psgpu_export_polympus and the
// blocking psgpu_polygonize_mpus): the compact mesh packed on the device into pinned staging,
// then scattered by host threads into the reference's PolyMPUs layout.  A group stages and
// scatters its parts through the same steps (psgpu_group.cpp; declared in psgpu_internal.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <thread>

#include "../../include/parsip_gpu.h"
#include "psgpu_internal.h"
#include "psgpu_launch.h"

using namespace psgpu;

namespace psgpu {
// The blocking export (Polygonize :360-371 into PolyMPUs, and the MPUSTATS of :372-376): one
// batch of async copies of the compact mesh, offsets, S1 flags and (for stats) counts into the
// context's pinned staging buffer (export_stage), one wait, then the host scatter
// (export_scatter).  Pageable destinations would cost a staged copy and a wait each (7 of
// them for a mesh plus statistics).  A group stages every part before it scatters the first,
// so the later parts' copies overlap the earlier parts' scatter.  Call after psgpu_finish.
int export_stage(psgpu_ctx* c, bool mesh, bool stats, ExportStage* st, hipEvent_t after) {
    const PsMeshInfo& I = c->info;
    ExportStage& S = *st;
    S.mesh = mesh;
    S.stats = stats;
    S.V = mesh ? I.ctVertices : 0;
    S.T = mesh ? I.ctTriangles : 0;
    S.N = c->mpuCount;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t N = S.N, V = S.V, T = S.T;
    // The per-piece flags sit at the front of the staging, at an offset no call moves: those
    // words only ever hold flags (an older call's epoch, or 0), never mesh or offset words, so
    // no stale word can equal this call's epoch (r04 kept them behind the mesh, where a call
    // with a smaller mesh found the previous call's packed triangles and offsets -- ADVICE r04)
    const size_t flagBytes = 4 * (size_t)kExportPieces * kExportPackBlocks * kExportFlagStride;
    S.oFlags = 0;
    S.oOffs = up(flagBytes);
    S.oPass = up(S.oOffs + (N + 1) * 8);
    S.oCnt = up(S.oPass + N);
    S.oMesh = up(S.oCnt + (stats ? N * 8 : 0));
    // the packed mesh: pack_words per piece; bounded by 4 extra words per piece
    S.meshBytes = mesh ? 4 * (pack_words(V, T) + 4 * kExportPieces) : 0;
    const size_t total = up(S.oMesh + S.meshBytes);
    if (total > c->hostStage.cap) {
        // coherent: the export kernels write it directly over PCIe
        PSGPU_CHECK(c->hostStage.reserve(total + total / 4, hipHostMallocMapped | hipHostMallocCoherent));
        memset(c->hostStage, 0, c->hostStage.cap);  // no stale flag can equal an epoch
    }
    if (++c->exportEpoch == 0) {  // wrapped: clear every old flag
        memset(c->hostStage, 0, c->hostStage.cap);
        c->exportEpoch = 1;
    }
    S.epoch = c->exportEpoch;
    unsigned char* h = c->hostStage;
    if (c->debug & (1 << 23)) {  // test hook: every word past the flags reads as this call's epoch
        // (the stream is idle: the previous export's scatter synchronised with it)
        uint32_t* w = reinterpret_cast<uint32_t*>(h + flagBytes);
        for (size_t i = 0, n = (c->hostStage.cap - flagBytes) / 4; i < n; ++i) w[i] = S.epoch;
    }
    hipStream_t s = c->stream;
    for (Event& e : c->exportEv) PSGPU_CHECK(e.create(hipEventDisableTiming));
    unsigned char* hd = nullptr;  // the staging as the device addresses it
    PSGPU_CHECK(hipHostGetDevicePointer(reinterpret_cast<void**>(&hd), h, 0));
    if (N) {
        MetaSrc ms{mesh ? c->offs : nullptr, c->passed, stats ? c->counts : nullptr, (uint32_t)N,
                   S.oOffs, S.oPass, S.oCnt};
        PSGPU_CHECK(launch_export_meta(ms, hd, s));
    }
    PSGPU_CHECK(hipEventRecord(c->exportEv[0], s));
    // the mesh packed piece by piece (MPU ranges of about 1 MB of mesh, at most 16: C3 0.535 vs
    // 0.570 ms with 2 MB) into one contiguous region by one kernel writing it over PCIe; the
    // host scatter of one piece overlaps the transfer of the next
    // 256 blocks: one wave per SIMD keeps the link busy; 1,024 or 2,048 were 1.8-4.5x slower,
    // every block's per-piece release (an L2 write-back) adding up (r04)
    S.packBlocks = kExportPackBlocks;
    S.pieces = (int)std::min<size_t>({(size_t)kExportPieces, std::max<size_t>(N, 1),
                                      1 + 4 * pack_words(V, T) / kExportPieceBytes});
    if (after) PSGPU_CHECK(hipStreamWaitEvent(s, after, 0));
    if (S.meshBytes && N) {
        PackSrc src{c->offs, c->pos, c->nrm, c->col, c->tris, (uint32_t)N, (uint32_t)S.pieces,
                    reinterpret_cast<uint32_t*>(hd + S.oFlags), S.epoch, S.packBlocks,
                    // test hook: the last block waits ~40 us before each piece's share
                    (c->debug & (1 << 24)) ? S.packBlocks - 1u : 0xffffffffu, 4000u};
        PSGPU_CHECK(launch_export_pack(src, reinterpret_cast<uint32_t*>(hd + S.oMesh), s));
    }
    PSGPU_CHECK(hipEventRecord(c->exportEv[1], s));
    return PSGPU_RET_SUCCESS;
}

int ScatterJob::prepare(psgpu_ctx* ctx, const ExportStage& st, PsMPU* out) {
    c = ctx;
    S = &st;
    mpus = out;
    PSGPU_CHECK(hipEventSynchronize(c->exportEv[0]));  // offsets, S1 flags, counts
    const unsigned char* h = c->hostStage;
    off = reinterpret_cast<const uint64_t*>(h + st.oOffs);
    passed = h + st.oPass;
    mesh = h + st.oMesh;
    flags = reinterpret_cast<const uint32_t*>(h + st.oFlags);
    side = c->cs * (float)PSGPU_CELLS_PER_MPU;
    active = out && st.mesh && !(c->debug & (1 << 22));  // bit 22: the transfers without the scatter
    if (!active) return PSGPU_RET_SUCCESS;
    // the pieces' MPU ranges and their places in the packed mesh (as k_export_pack laid them out)
    const size_t N = st.N;
    size_t base = 0;
    for (int k = 0; k <= st.pieces; ++k) pm[k] = (uint32_t)((uint64_t)N * (uint64_t)k / (uint64_t)st.pieces);
    for (int k = 0; k < st.pieces; ++k) {
        pv0[k] = (uint32_t)off[pm[k]];
        pt0[k] = (uint32_t)(off[pm[k]] >> 32);
        pnv[k] = (uint32_t)off[pm[k + 1]] - pv0[k];
        pbase[k] = base;
        base += 4 * pack_words(pnv[k], (uint32_t)(off[pm[k + 1]] >> 32) - pt0[k]);
    }
    return PSGPU_RET_SUCCESS;
}

// piece k is in when every block of k_export_pack has raised its flag for it; the kernel's
// event ends the wait should it fail.  One thread at a time reads the flags (they sit in
// memory the device writes over PCIe: sixteen threads polling them slowed the device's
// writes in some calls) and publishes the count of pieces in; the others watch that count.
bool ScatterJob::wait_piece(int k) {
    for (uint32_t spin = 1;; ++spin) {
        const int r = ready.load(std::memory_order_acquire);
        if (r > k) return true;
        if (r < 0) return false;  // the kernel failed
        bool idle = false;
        if (polling.compare_exchange_strong(idle, true, std::memory_order_acq_rel)) {
            int n = ready.load(std::memory_order_acquire);
            while (n >= 0 && n < S->pieces) {  // advance over every piece already in
                const uint32_t* f = flags + (size_t)n * S->packBlocks * kExportFlagStride;
                // from the first flag not yet seen up: every read of a flag still down is a read
                // of a line the device is about to write (one flag a line, kExportFlagStride)
                uint32_t b = pollBlock;
                while (b < S->packBlocks && __atomic_load_n(f + (size_t)b * kExportFlagStride, __ATOMIC_ACQUIRE) == S->epoch) ++b;
                pollBlock = b;
                if (b < S->packBlocks) {
                    if ((spin & 63) == 0) {
                        const hipError_t e = hipEventQuery(c->exportEv[1]);
                        if (e != hipErrorNotReady) {  // done (every flag must be up) or failed
                            while (b < S->packBlocks && __atomic_load_n(f + (size_t)b * kExportFlagStride, __ATOMIC_ACQUIRE) == S->epoch) ++b;
                            if (e != hipSuccess || b < S->packBlocks) n = -1;
                            else ++n;
                            pollBlock = 0;
                            ready.store(n, std::memory_order_release);
                            continue;
                        }
                    }
                    break;
                }
                if (trace) tPiece[n] = now_ns();
                pollBlock = 0;
                ready.store(++n, std::memory_order_release);
            }
            polling.store(false, std::memory_order_release);
            for (int i = 0; i < 256; ++i) __builtin_ia32_pause();  // ~1-2 us between reads of the flags
        }
        std::this_thread::yield();
    }
}

// MPUs [lb, le) into PolyMPUs (Polygonize :360-371); `have` = the pieces this thread has seen in
bool ScatterJob::range(uint32_t lb, uint32_t le, int* have) {
    int k = 0;
    while (k + 1 < S->pieces && lb >= pm[k + 1]) ++k;
    for (uint32_t l = lb; l < le; ++l) {
        while (k + 1 < S->pieces && l >= pm[k + 1]) ++k;
        const uint32_t v0 = (uint32_t)off[l], nv = (uint32_t)off[l + 1] - v0;
        const uint32_t t0 = (uint32_t)(off[l] >> 32), nt = (uint32_t)(off[l + 1] >> 32) - t0;
        const unsigned char* P = mesh + pbase[k];
        const float* pos = reinterpret_cast<const float*>(P) + 3 * (v0 - pv0[k]);
        const float* nrm = reinterpret_cast<const float*>(P + pnv[k] * 12) + 3 * (v0 - pv0[k]);
        const float* col = reinterpret_cast<const float*>(P + pnv[k] * 24) + 3 * (v0 - pv0[k]);
        const uint16_t* tri = reinterpret_cast<const uint16_t*>(P + pnv[k] * 36) + 3 * (t0 - pt0[k]);
        while (*have <= k) {  // this MPU's piece written (the pieces come in order)
            if (!wait_piece(*have)) return false;
            ++*have;
        }
        const uint32_t m = c->mpuBegin + l;
        const uint32_t kk = m % c->dims[2], j = (m / c->dims[2]) % c->dims[1], i = m / (c->dims[2] * c->dims[1]);
        PsMPU& M = mpus[l];
        M.bboxLo.x = c->primsHost.bboxLo.x + (float)i * side;
        M.bboxLo.y = c->primsHost.bboxLo.y + (float)j * side;
        M.bboxLo.z = c->primsHost.bboxLo.z + (float)kk * side;
        M.ctFieldEvals = passed[l] ? 128 : 0;
        M.ctVertices = (uint16_t)nv;
        M.ctTriangles = (uint16_t)nt;
        memcpy(M.vPos, pos, (size_t)nv * 12);
        memcpy(M.vNorm, nrm, (size_t)nv * 12);
        memcpy(M.vColor, col, (size_t)nv * 12);
        memcpy(M.triangles, tri, (size_t)nt * 6);
    }
    return true;
}

// thread k of nth: chunks of 128 MPUs dealt round robin (the surface lies in a few slabs of
// the range), in ascending order, so the pieces are waited for in the order they come
void ScatterJob::task(unsigned k, unsigned nth) {
    if (!active) return;
    if (trace) {
        int64_t z = 0;
        (void)tFirstTask.compare_exchange_strong(z, now_ns());
    }
    int have = 0;
    const uint32_t N = (uint32_t)S->N;
    for (uint32_t b = k * 128u; b < N; b += nth * 128u)
        if (!range(b, std::min<uint32_t>(N, b + 128u), &have)) {
            failed = true;
            return;
        }
}

int ScatterJob::finish(PsMpuStats* stats) {
    if (failed) return PSGPU_RET_DEVICE_ERROR;
    PSGPU_CHECK(hipStreamSynchronize(c->stream));  // the packing kernel done
    if (stats && S->stats) {
        const uint64_t* cnt = reinterpret_cast<const uint64_t*>(c->hostStage + S->oCnt);
        memset(stats, 0, sizeof(PsMpuStats) * S->N);
        for (uint32_t l = 0; l < S->N; ++l) {
            PsMpuStats& st = stats[l];
            if (passed[l]) {
                st.passedPrecheck = 1;
                st.ctFieldEvals = 128;
            }
            st.ctVertices = (uint32_t)(cnt[l] & 0xffffffffu);
            st.ctTriangles = (uint32_t)(cnt[l] >> 32);
        }
    }
    return PSGPU_RET_SUCCESS;
}

// The scatter is bound by the write-allocates of the sparse PolyMPUs layout (21.5 KB per MPU):
// several host threads, as the reference's TBB bodies fill it -- about one per 256 KB of mesh,
// at most 16 (C3 0.535 vs 0.586 ms with 8), kept in c's pool.  Runs jobs[0..n) in one pass: every thread takes its chunks of
// each job in turn.
int scatter_jobs(psgpu_ctx* c, ScatterJob* jobs, size_t n) {
    size_t bytes = 0;
    for (size_t j = 0; j < n; ++j) bytes += jobs[j].active ? jobs[j].S->meshBytes : 0;
    const unsigned nth = (unsigned)std::min<size_t>({16, std::max(1u, std::thread::hardware_concurrency()),
                                                    1 + bytes / (256 << 10)});
    std::function<void(unsigned)> task = [&](unsigned k) {
        for (size_t j = 0; j < n; ++j) jobs[j].task(k, nth);
    };
    // nth workers on the caller's NUMA node; the caller only waits
    if (nth > 1 && (!c->scatterPool || c->scatterPool->workers() < nth)) {
        c->scatterPool.reset();
        try {
            cpu_set_t node;
            const bool haveNode = ScatterPool::caller_node_cpus(&node);
            c->scatterPool.reset(new ScatterPool(nth, haveNode ? &node : nullptr));
        } catch (...) {  // no threads to be had: this caller scatters alone
            c->scatterPool.reset();
        }
    }
    if (nth > 1 && c->scatterPool) c->scatterPool->run(nth, task, false);
    else
        for (unsigned k = 0; k < nth; ++k) task(k);
    return PSGPU_RET_SUCCESS;
}

// PSGPU_EXPORT_TRACE=1: every blocking export prints its phases (ms from the call's start) to
// stderr -- kernels done, packing enqueued, metadata in, first scatter task, each piece in,
// scatter done, end (tools/blocking_seq.py collects them)
bool export_trace_on() {
    static const bool on = [] {
        const char* e = getenv("PSGPU_EXPORT_TRACE");
        return e && *e && *e != '0';
    }();
    return on;
}

int export_scatter(psgpu_ctx* c, const ExportStage& S, PsMPU* mpus, PsMpuStats* stats, const int64_t* tr) {
    ScatterJob job;
    job.trace = tr != nullptr;
    int rc = job.prepare(c, S, mpus);
    const int64_t tPrep = tr ? now_ns() : 0;
    if (rc == PSGPU_RET_SUCCESS) rc = scatter_jobs(c, &job, 1);
    const int64_t tScat = tr ? now_ns() : 0;
    if (rc == PSGPU_RET_SUCCESS) rc = job.finish(stats);
    if (tr) {
        const int64_t t0 = tr[0], tEnd = now_ns();
        auto ms = [t0](int64_t t) { return t ? (double)(t - t0) * 1e-6 : -1.0; };
        fprintf(stderr, "psgpu export: mpus %zu V %zu pieces %d | kernels %.3f packing %.3f meta %.3f first_task %.3f pieces",
                S.N, S.V, S.pieces, ms(tr[1]), ms(tr[2]), ms(tPrep), ms(job.tFirstTask.load()));
        for (int k = 0; k < S.pieces; ++k) fprintf(stderr, " %.3f", ms(job.tPiece[k]));
        fprintf(stderr, " | scatter %.3f end %.3f\n", ms(tScat), ms(tEnd));
    }
    return rc;
}

int export_blocking(psgpu_ctx* c, PsMPU* mpus, uint32_t capacity, uint32_t* outCt, PsMpuStats* stats, int64_t tCall) {
    int64_t tr[3] = {tCall ? tCall : now_ns(), 0, 0};
    const bool trace = export_trace_on();
    PsMeshInfo I;
    int rc = finished_run(c, &I);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    tr[1] = now_ns();
    if (outCt) *outCt = c->mpuCount;
    if (mpus) {
        if (c->mpuCount > capacity) return PSGPU_RET_MPU_OVERFLOW;
        if (I.firstOverflowMPU >= 0) return PSGPU_RET_MPU_VT_OVERFLOW;
    }
    if (!mpus && !stats) return PSGPU_RET_PARAM_ERROR;
    ExportStage st;
    rc = export_stage(c, mpus != nullptr, stats != nullptr, &st);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    tr[2] = now_ns();
    return export_scatter(c, st, mpus, stats, trace ? tr : nullptr);
}
}  // namespace psgpu

extern "C" {

int psgpu_export_polympus(psgpu_ctx* c, PsMPU* mpus, uint32_t capacity, uint32_t* outCt) {
    if (!mpus) {  // the count (and overflow) check alone
        PsMeshInfo I;
        int rc = psgpu_finish(c, &I);
        if (rc != PSGPU_RET_SUCCESS) return rc;
        if (outCt) *outCt = c->mpuCount;
        if (c->mpuCount > capacity) return PSGPU_RET_MPU_OVERFLOW;
        if (I.firstOverflowMPU >= 0) return PSGPU_RET_MPU_VT_OVERFLOW;
        return PSGPU_RET_PARAM_ERROR;
    }
    return export_blocking(c, mpus, capacity, outCt, nullptr);
}

}  // extern "C"
