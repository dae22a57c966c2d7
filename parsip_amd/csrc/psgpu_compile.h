// psgpu_compile.h — the owner of a compile that runs on a host thread (host only: no HIP, no
// hiprtc).  A compile never outlives the context that started it: every context keeps its
// compiles in a CompileSlot, and the slot's destructor waits for them.
#pragma once
#include <algorithm>
#include <chrono>
#include <future>
#include <optional>
#include <utility>
#include <vector>

namespace psgpu {

// At most one pending job with result R, and the retired jobs that still run.  A hiprtc thread
// left running into process exit can outlive the compiler's own lazily built statics (a core
// dump after a run that changed options under a compile): no job is let go before it has ended.
template <typename R>
struct CompileSlot {
    using Future = std::shared_future<R>;

    CompileSlot() = default;
    CompileSlot(const CompileSlot&) = delete;
    CompileSlot& operator=(const CompileSlot&) = delete;
    ~CompileSlot() { drain(); }

    bool pending() const { return cur.valid(); }
    size_t held() const { return (cur.valid() ? 1 : 0) + retired.size(); }  // pending + retired (tests)

    // f becomes the pending job; one pending already is retired.  Never blocks.
    void start(Future f) {
        drop();
        cur = std::move(f);
    }
    // Retire the pending job: it finishes in the background.  Never blocks.
    void drop() {
        if (cur.valid()) retired.push_back(std::move(cur));
        cur = Future();
        retired.erase(std::remove_if(retired.begin(), retired.end(), ready), retired.end());  // forget the finished
    }
    // The pending job's result once it is ready (wait: block for it), leaving none pending;
    // otherwise nothing, and nothing changes.
    std::optional<R> poll(bool wait) {
        if (!cur.valid() || (!wait && !ready(cur))) return std::nullopt;
        std::optional<R> r(cur.get());
        cur = Future();
        return r;
    }
    // Wait for the pending job and every retired one; the slot is empty afterwards.
    void drain() {
        if (cur.valid()) cur.wait();
        cur = Future();
        for (Future& f : retired) f.wait();
        retired.clear();
    }

private:
    static bool ready(const Future& f) { return f.wait_for(std::chrono::seconds(0)) == std::future_status::ready; }
    Future cur;
    std::vector<Future> retired;
};

}  // namespace psgpu
