// psgpu_comm.cpp — the multi-process form of a group (C-ABI, include/parsip_gpu.h): one process
// per GPU (torchrun / MPI launchers), each rank owns a range of the same split (computed
// identically on every rank) and the parts' totals are exchanged with one RCCL all-gather of 8
// words per rank on the context's stream, right after its k_finish (stream-ordered, no host
// round trip inside a frame).  A rank's range may itself run as a group of parts on its one
// device (psgpu_group.cpp), which this file reaches through the public psgpu_group_* calls only.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "psgpu_group_plan.h"
#include "psgpu_internal.h"
#include "psgpu_launch.h"

using namespace psgpu;

struct psgpu_comm {
    ncclComm_t comm = nullptr;
    int nranks = 0, rank = 0, device = 0;
    DevBuf<uint32_t> gathered;         // device: nranks x 8 words
    PinnedBuf<uint32_t> hostGathered;  // pinned copy
    DevBuf<uint32_t> flag;             // device: the "some rank re-ran" all-reduce word, then a
                                       // constant 2 (a failed rank's contribution, no copy needed)
    PinnedBuf<uint32_t> hostFlag;      // pinned
    bool pending = false;
    bool reexchanged = false;          // the last result needed the second exchange
    psgpu_ctx* ctx = nullptr;          // the context whose run was exchanged
    psgpu_group* group = nullptr;      // or the group whose parts were summed:
    std::vector<Event> done;           // per part, what part 0's stream waits for (made on first use)
    DevBuf<uint32_t> sumTotals;        // the parts' 8 words, summed
};

static int nccl_fail(ncclResult_t r, const char* what) {
    if (r == ncclSuccess) return PSGPU_RET_SUCCESS;
    fprintf(stderr, "psgpu: %s failed: %s\n", what, ncclGetErrorString(r));
    return PSGPU_RET_DEVICE_ERROR;
}

static hipStream_t run_stream(const psgpu_ctx* c) { return c->runStream ? c->runStream : (hipStream_t)c->stream; }

// The totals of the group's parts, summed into m->sumTotals on `stream` (the comm's device current).
static hipError_t sum_parts(psgpu_comm* m, psgpu_group* g, hipStream_t stream) {
    TotalsParts tp{};
    tp.n = psgpu_group_size(g);
    for (int k = 0; k < tp.n; ++k) tp.p[k] = psgpu_group_context(g, k)->totals;
    return launch_sum_totals(tp, m->sumTotals, stream);
}

extern "C" {

int psgpu_comm_unique_id(uint8_t id[PSGPU_COMM_ID_BYTES]) {
    static_assert(sizeof(ncclUniqueId) == PSGPU_COMM_ID_BYTES, "ncclUniqueId size");
    if (!id) return PSGPU_RET_PARAM_ERROR;
    ncclUniqueId u;
    const int rc = nccl_fail(ncclGetUniqueId(&u), "ncclGetUniqueId");
    if (rc == PSGPU_RET_SUCCESS) memcpy(id, &u, sizeof(u));
    return rc;
}

int psgpu_comm_create(psgpu_ctx* ctx, const uint8_t id[PSGPU_COMM_ID_BYTES], int nranks, int rank,
                      psgpu_comm** out) {
    if (!ctx || !id || !out || nranks <= 0 || rank < 0 || rank >= nranks) return PSGPU_RET_PARAM_ERROR;
    *out = nullptr;
    int rc = set_device(ctx);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    psgpu_comm* m = new psgpu_comm();
    m->nranks = nranks;
    m->rank = rank;
    m->device = ctx->device;
    ncclUniqueId u;
    memcpy(&u, id, sizeof(u));
    rc = nccl_fail(ncclCommInitRank(&m->comm, nranks, u, rank), "ncclCommInitRank");
    if (rc == PSGPU_RET_SUCCESS &&
        (m->gathered.reserve((size_t)nranks * 8, Growth::Exact) != hipSuccess ||
         m->hostGathered.reserve((size_t)nranks * 8, hipHostMallocDefault) != hipSuccess ||
         m->flag.reserve(2, Growth::Exact) != hipSuccess ||
         m->hostFlag.reserve(9, hipHostMallocDefault) != hipSuccess))
        rc = PSGPU_RET_DEVICE_ERROR;
    if (rc == PSGPU_RET_SUCCESS) {
        const uint32_t failWords[2] = {0u, 2u};
        if (hipMemcpy(m->flag, failWords, sizeof(failWords), hipMemcpyHostToDevice) != hipSuccess)
            rc = PSGPU_RET_DEVICE_ERROR;
    }
    if (rc != PSGPU_RET_SUCCESS) {
        psgpu_comm_destroy(m);
        return rc;
    }
    *out = m;
    return PSGPU_RET_SUCCESS;
}

void psgpu_comm_destroy(psgpu_comm* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (m->comm) (void)ncclCommDestroy(m->comm);
    delete m;  // with its buffers and events
}

// Enqueue the exchange of the context's last polygonization (its k_finish totals) on the
// context's stream: ncclAllGather of 8 words per rank (psgpu_comm_result copies them to the host).
int psgpu_comm_exchange(psgpu_comm* m, psgpu_ctx* ctx) {
    if (!m || !m->comm || !ctx || ctx->device != m->device) return PSGPU_RET_PARAM_ERROR;
    int rc = set_device(ctx);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    rc = nccl_fail(ncclAllGather(ctx->totals, m->gathered, 8, ncclUint32, m->comm, run_stream(ctx)), "ncclAllGather");
    if (rc != PSGPU_RET_SUCCESS) return rc;
    m->pending = true;
    m->ctx = ctx;
    m->group = nullptr;
    return PSGPU_RET_SUCCESS;
}

// The same for a rank whose range runs as a group of parts on its one device (several
// streams): part 0's stream waits for the others' last launches, sums their totals and
// all-gathers the sum.
int psgpu_comm_exchange_group(psgpu_comm* m, psgpu_group* g) {
    const int n = psgpu_group_size(g);
    if (!m || !m->comm || n <= 0 || n > 16) return PSGPU_RET_PARAM_ERROR;
    for (int k = 0; k < n; ++k)
        if (psgpu_group_context(g, k)->device != m->device) return PSGPU_RET_PARAM_ERROR;
    psgpu_ctx* c0 = psgpu_group_context(g, 0);
    int rc = set_device(c0);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    m->done.resize((size_t)n);
    PSGPU_CHECK(m->sumTotals.reserve(8, Growth::Exact));
    hipStream_t s0 = run_stream(c0);
    for (int k = 0; k < n; ++k) {
        hipStream_t sk = run_stream(psgpu_group_context(g, k));
        if (sk != s0) {
            PSGPU_CHECK(m->done[k].create(hipEventDisableTiming));
            PSGPU_CHECK(hipEventRecord(m->done[k], sk));
            PSGPU_CHECK(hipStreamWaitEvent(s0, m->done[k], 0));
        }
    }
    PSGPU_CHECK(sum_parts(m, g, s0));
    rc = nccl_fail(ncclAllGather(m->sumTotals, m->gathered, 8, ncclUint32, m->comm, s0), "ncclAllGather");
    if (rc != PSGPU_RET_SUCCESS) return rc;
    m->pending = true;
    m->ctx = c0;
    m->group = g;
    return PSGPU_RET_SUCCESS;
}

// After the exchange: every rank's part (MPU range from the gathered counts, bases in
// rank order) and the totals over all ranks.  Finishes the context.  finish() re-runs a
// polygonization whose buffers or k_mpu grid fell short, after its totals were already
// exchanged; whether any rank did so is itself agreed collectively (an all-reduce MAX of a
// flag, on every rank), and then EVERY rank exchanges again -- a collective entered by only
// the ranks that re-ran would block them forever and leave the others with stale counts.
// A rank whose finish fails still enters the all-reduce, with flag 2: then every rank
// returns an error (its own, or PSGPU_RET_DEVICE_ERROR for another rank's failure) and
// none waits for a collective the failed rank will not enter.
// If even that cannot be prepared (the device cannot be made current, or the flag cannot be
// copied to it), the rank still enters the all-reduce, from the constant 2 kept beside the flag
// (no copy needed); should the collective itself fail to enqueue (on this path or on the
// normal one), the communicator is aborted (ncclCommAbort) and unusable from then on --
// psgpu_comm_destroy is all that is left to call.
int psgpu_comm_result(psgpu_comm* m, PsMeshInfo* totalOut, PsGroupPart* partsOut) {
    if (!m || !m->pending || !m->ctx || !m->comm) return PSGPU_RET_PARAM_ERROR;
    psgpu_ctx* c = m->ctx;
    PsMeshInfo mine;
    int local = m->group ? psgpu_group_finish(m->group, &mine, nullptr) : psgpu_finish(c, &mine);
    m->pending = false;
    hipStream_t s = run_stream(c);
    auto enter_failed = [&](int rc) {  // this rank's flag 2, so that no other rank waits forever
        if (ncclAllReduce(m->flag + 1, m->flag, 1, ncclUint32, ncclMax, m->comm, s) != ncclSuccess ||
            hipStreamSynchronize(s) != hipSuccess) {
            (void)ncclCommAbort(m->comm);
            m->comm = nullptr;
        }
        return rc;
    };
    if (hipSetDevice(m->device) != hipSuccess) return enter_failed(local != PSGPU_RET_SUCCESS ? local : PSGPU_RET_DEVICE_ERROR);
    const size_t gb = (size_t)m->nranks * 8 * sizeof(uint32_t);
    uint32_t flag = 2u;
    if (local == PSGPU_RET_SUCCESS) {
        // this rank's totals as exchanged vs the totals of its final run (all 8 words: counts,
        // the first overflowing MPU, the error word), both to the host in one wait; the
        // gathered words come to the host only here (not per step: one HIP call less on the
        // host's enqueue path, which bounds small rank shares)
        const uint32_t* finalWords = c->totals;
        if (m->group) {  // the exchange was exchange_group's: the parts' final totals, summed as there
            if (sum_parts(m, m->group, s) != hipSuccess) local = PSGPU_RET_DEVICE_ERROR;
            finalWords = m->sumTotals;
        }
        if (local == PSGPU_RET_SUCCESS &&
            (hipMemcpyAsync(m->hostGathered, m->gathered, gb, hipMemcpyDeviceToHost, s) != hipSuccess ||
             hipMemcpyAsync(m->hostFlag + 1, finalWords, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, s) != hipSuccess ||
             hipStreamSynchronize(s) != hipSuccess))
            local = PSGPU_RET_DEVICE_ERROR;
        if (local == PSGPU_RET_SUCCESS)
            flag = memcmp(m->hostGathered + 8 * m->rank, m->hostFlag + 1, 8 * sizeof(uint32_t)) != 0 ? 1u : 0u;
    }
    *m->hostFlag = flag;
    if (hipMemcpyAsync(m->flag, m->hostFlag, sizeof(uint32_t), hipMemcpyHostToDevice, s) != hipSuccess)
        return enter_failed(local != PSGPU_RET_SUCCESS ? local : PSGPU_RET_DEVICE_ERROR);
    int rc = nccl_fail(ncclAllReduce(m->flag, m->flag, 1, ncclUint32, ncclMax, m->comm, s), "ncclAllReduce");
    if (rc != PSGPU_RET_SUCCESS) {  // the other ranks may be inside the all-reduce: abort it for them
        (void)ncclCommAbort(m->comm);
        m->comm = nullptr;
        return local != PSGPU_RET_SUCCESS ? local : rc;
    }
    PSGPU_CHECK(hipMemcpyAsync(m->hostFlag, m->flag, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    PSGPU_CHECK(hipStreamSynchronize(s));
    if (local != PSGPU_RET_SUCCESS) return local;
    if (*m->hostFlag >= 2u) return PSGPU_RET_DEVICE_ERROR;  // another rank's finish failed
    m->reexchanged = *m->hostFlag != 0u;
    if (m->reexchanged) {  // some rank's totals changed after the exchange: all ranks exchange again
        rc = m->group ? psgpu_comm_exchange_group(m, m->group) : psgpu_comm_exchange(m, c);
        if (rc != PSGPU_RET_SUCCESS) return rc;
        PSGPU_CHECK(hipMemcpyAsync(m->hostGathered, m->gathered, gb, hipMemcpyDeviceToHost, s));
        PSGPU_CHECK(hipStreamSynchronize(s));
    }
    m->pending = false;
    const size_t n = (size_t)m->nranks;
    std::vector<PsMeshInfo> info(n);
    std::vector<uint32_t> vBase(n), tBase(n);
    for (size_t r = 0; r < n; ++r) {
        const uint32_t* w = m->hostGathered + 8 * r;
        if (w[7]) return PSGPU_RET_DEVICE_ERROR;  // a rank's device protocol error
        info[r] = decode_totals(w);
    }
    PsMeshInfo T;
    rc = place_parts(info.data(), n, vBase.data(), tBase.data(), &T);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    uint32_t mb = 0;
    for (size_t r = 0; partsOut && r < n; ++r) {
        PsGroupPart& P = partsOut[r];
        memset(&P, 0, sizeof(P));
        P.device = (int)r == m->rank ? c->device : -1;
        P.mpuBegin = mb;
        P.mpuEnd = mb += info[r].ctMPUs;
        P.vertexBase = vBase[r];
        P.triangleBase = tBase[r];
        P.info = info[r];
    }
    if (totalOut) *totalOut = T;
    return PSGPU_RET_SUCCESS;
}

int psgpu_comm_reexchanged(psgpu_comm* m) { return (m && m->reexchanged) ? 1 : 0; }

}  // extern "C"
