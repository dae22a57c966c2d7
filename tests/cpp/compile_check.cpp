// The owner of a pending compile (parsip_amd/csrc/psgpu_compile.h), host only: start and drop
// never wait, poll hands a result out once, drain and the destructor wait for the pending job
// and for every retired one.  A job is a std::async task that blocks on a gate the test opens
// and sets a flag when it ends: a call that wrongly waits on a closed gate hangs (the caller's
// time limit reports it).  No sleeps, no timing.
#include <atomic>
#include <cstdio>
#include <future>
#include <thread>

#include "psgpu_compile.h"

namespace {

struct Job {
    std::promise<void> gate;
    std::atomic<bool> done{false};
    std::shared_future<int> fut;  // the test's own copy: fut.wait() is "the job has ended"
    explicit Job(int value) {
        fut = std::async(std::launch::async, [this, value, g = gate.get_future().share()] {
                  g.wait();
                  done.store(true);
                  return value;
              }).share();
    }
    void open() { gate.set_value(); }
};

int g_line = 0;
#define CHECK(x)                     \
    do {                             \
        if (!(x) && !g_line) {       \
            g_line = __LINE__;       \
            std::printf("line %d: %s\n", __LINE__, #x); \
        }                            \
    } while (0)

using Slot = psgpu::CompileSlot<int>;

void start_under_pending_and_drop() {
    Job a(1), b(2), c(3);
    Slot s;
    s.start(a.fut);
    s.start(b.fut);  // a's gate is closed: this returns all the same
    CHECK(!a.done.load() && s.pending() && s.held() == 2);  // a is retired, not lost
    a.open();
    a.fut.wait();
    s.drop();  // b retired, a forgotten
    CHECK(!s.pending() && s.held() == 1);
    CHECK(!s.poll(true).has_value());  // nothing pending: nothing to wait for
    CHECK(!b.done.load() && s.held() == 1);
    b.open();
    b.fut.wait();
    s.start(c.fut);  // b forgotten
    CHECK(s.pending() && s.held() == 1);
    c.open();
    const std::optional<int> r = s.poll(true);
    CHECK(r.has_value() && *r == 3 && c.done.load());
    CHECK(!s.pending() && s.held() == 0);
}

void poll_without_waiting() {
    Job a(7);
    Slot s;
    s.start(a.fut);
    CHECK(!s.poll(false).has_value());
    CHECK(s.pending() && s.held() == 1 && !a.done.load());
    a.open();
    a.fut.wait();
    const std::optional<int> r = s.poll(false);
    CHECK(r.has_value() && *r == 7);
    CHECK(!s.pending() && s.held() == 0);
    CHECK(!s.poll(false).has_value() && !s.poll(true).has_value());  // exactly once
}

// one pending job and two retired ones, their gates opened from another thread
void drain_and_destructor(bool byDestructor) {
    Job a(1), b(2), c(3);
    std::thread opener;
    {
        Slot s;
        s.start(a.fut);
        s.start(b.fut);
        s.start(c.fut);
        CHECK(s.held() == 3);
        opener = std::thread([&] {
            a.open();
            b.open();
            c.open();
        });
        if (!byDestructor) {
            s.drain();
            CHECK(a.done.load() && b.done.load() && c.done.load());
            CHECK(!s.pending() && s.held() == 0);
            s.drain();  // twice: nothing left to wait for
            CHECK(s.held() == 0);
        }
    }
    CHECK(a.done.load() && b.done.load() && c.done.load());
    opener.join();
}

void never_used() {
    Slot s;
    CHECK(!s.pending() && s.held() == 0);
    CHECK(!s.poll(false).has_value() && !s.poll(true).has_value());
    s.drop();
    s.drain();
    s.drain();
    CHECK(!s.pending() && s.held() == 0);
}

}  // namespace

int main() {
    start_under_pending_and_drop();
    poll_without_waiting();
    drain_and_destructor(false);
    drain_and_destructor(true);
    never_used();
    { Slot unused; }
    if (g_line) return 1;
    std::printf("ok\n");
    return 0;
}
