// psgpu_jit.h — run-time specialised tree-walk kernels (hiprtc), see psgpu_jit.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <vector>

#include "psgpu_compile.h"
#include "psgpu_model.h"

namespace psgpu {

struct JitKernels {
    hipModule_t mod = nullptr;
    hipFunction_t precheck = nullptr, mpu = nullptr, vertex = nullptr, vertexW = nullptr, finish = nullptr,
                  finishQ = nullptr, finishP = nullptr, probe = nullptr;
    hipFunction_t precheckS = nullptr, mpuS = nullptr;  // tree split at the root (two waves per item)
    hipFunction_t surface = nullptr;  // k_vertex + k_finish in one launch (small launches; with the split kernels)
    hipFunction_t surfaceW = nullptr;  // the same with one lane per vertex (PSGPU_OPT_FUSED_SURFACE 3)
    hipFunction_t front = nullptr, frontS = nullptr;  // k_precheck + k_mpu in one launch (k_front; unsplit / split)
};

extern const char* const kJitArch;  // "gfx950"

// A compiled code object (or the compiler's error) for one generated source.
struct JitCode {
    std::string key;         // source + embedded headers + tuning + toolchain
    std::vector<char> code;  // empty on failure
    std::string error;
};
using JitSlot = CompileSlot<std::shared_ptr<const JitCode>>;
using JitFuture = JitSlot::Future;

// A polygonizer context's run-time kernels and their compiles (psgpu_host.cpp: jit_start,
// jit_poll, tier_poll, tier_count).  PSGPU_OPT_JIT 3 (tiered): once the model has stayed
// unchanged for tierRuns runs, its baked kernels compile on a host thread and replace the
// structure kernels (kept in kernels1).
struct JitState {
    int use = 1;                          // PSGPU_OPT_JIT
    int async = 1;                        // set_model returns while hiprtc compiles (interpreter meanwhile)
    std::shared_ptr<JitKernels> kernels;  // specialised kernels of the current model
    std::string error;
    int tier = 0;                         // what `kernels` holds: 0 none, 1 structure, 2 baked kernels
    int tierRuns = 16;
    int staticRuns = 0;                   // runs of the current model on the structure kernels
    bool tier2Failed = false;             // the baked compile failed: stay on tier 1 for this model
    std::shared_ptr<JitKernels> kernels1;  // the structure kernels while tier 2 serves
    JitSlot compile;                      // the current model's kernels, while they compile
    JitSlot baked;                        // its baked tier
};

// Request the model's specialised kernels: hiprtc compiles on a host thread (one job per
// distinct source; an on-disk cache serves repeats unless useDisk is false).  No GPU needed.
// baked: primitive / op parameters compiled in as literals (recompiles when they change).
JitFuture jit_request(const DevModel& m, bool baked, bool useDisk = true, bool split = false);
// Load a finished code object on `device` (the calling thread's current device), cached
// per device; nullptr + *err on failure (a stale cached object is dropped from the cache).
std::shared_ptr<JitKernels> jit_load(const JitCode& code, int device, std::string* err);
// Compile (and cache) without loading: code-object size, or -1 and *err.  No GPU needed.
long jit_compile_only(const DevModel& m, bool baked, std::string* err, bool split = false);
// The generated HIP source (tests and debugging).
std::string jit_source(const DevModel& m, bool baked, bool split = false);
// the generated walk splits at the root (TreeEval::kSplit): a binary known op over two ops
bool jit_splittable(const DevModel& m);
// Compat mode: compile a generated compact-tree source (psgpu_gui_jit.cpp) against the
// embedded compat headers, with the same on-disk cache, on a host thread (jobs are neither
// deduplicated nor retained: an editor session makes a new source per edit); the second form
// waits for it.  No GPU needed.
JitFuture jit_request_gui(const std::string& src);
bool jit_compile_gui(const std::string& src, std::vector<char>& code, std::string* err);

}  // namespace psgpu
