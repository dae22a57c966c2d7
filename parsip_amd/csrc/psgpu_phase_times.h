// psgpu_phase_times.h — hipEvent times of a call's launch sequence (PSGPU_OPT_KERNEL_TIMING):
// what psgpu_weld_times, psgpu_weld_shells_times, psgpu_weld_filter_times and
// psgpu_group_weld_times report.  N phases: the whole call, then its N - 1 steps.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "psgpu_buf.h"

namespace psgpu {

// The events a shared launch sequence records, in order (PhaseTimes::rest); none when untimed.
struct PhaseCursor {
    Event* ev = nullptr;
    hipError_t mark(hipStream_t s) { return ev ? hipEventRecord(*ev++, s) : hipSuccess; }
};

template <int N>
struct PhaseTimes {
    Event ev[N];            // before the first step, after each; made by the first timed call
    float ms[N] = {};       // the last call's: the whole, then each step (0: untimed, or it launched nothing)
    bool timed = false;     // the call in progress records events; `next` is the first it has not
    int next = 0;

    void clear() {
        std::fill(ms, ms + N, 0.0f);
        timed = false;
        next = 0;
    }
    // A call begins; the events' device is current.
    hipError_t begin(bool on) {
        clear();
        for (Event& e : ev)
            if (on) {
                const hipError_t err = e.create();
                if (err != hipSuccess) return err;
            }
        timed = on;
        return hipSuccess;
    }
    hipError_t mark(hipStream_t s) { return timed ? hipEventRecord(ev[next++], s) : hipSuccess; }
    hipEvent_t take() { return timed ? ev[next++].h : nullptr; }  // for a callee that records one event itself
    PhaseCursor rest() { return PhaseCursor{timed ? ev + next : nullptr}; }  // ... or all that remain
    // The call's stream has been waited for and every event recorded.
    void collect() {
        if (!timed) return;
        (void)hipEventElapsedTime(&ms[0], ev[0], ev[N - 1]);
        for (int k = 1; k < N; ++k) (void)hipEventElapsedTime(&ms[k], ev[k - 1], ev[k]);
    }
    int report(float* out, int maxPhases, const char** names, const char* const* table) const {
        const int n = std::min(maxPhases, N);
        for (int k = 0; k < n; ++k) {
            if (out) out[k] = ms[k];
            if (names) names[k] = table[k];
        }
        return n;
    }
    void free() {
        for (Event& e : ev) e.reset();
        clear();
    }
};

}  // namespace psgpu
