/* serial_shim.h — TEST INFRASTRUCTURE ONLY.  A serial stand-in for the slice of the legacy
 * TBB API that PS_Polygonizer.{h,cpp} use, so the reference can be compiled
 * where no TBB headers exist (oracle/Makefile target `ref`).  TBB only schedules work there;
 * it touches no value.  Everything runs on the calling thread:
 *   - task_scheduler_observer::observe(true) calls on_scheduler_entry once, at once;
 *   - parallel_for runs the body over the whole range in one call;
 *   - enumerable_thread_specific holds at most one element, the caller's.
 * tbb_thread::id and tick_count keep the LP64 sizes of the real ones (a pthread_t and one
 * 64-bit count), so MPUSTATS keeps its 32-byte layout. */
#ifndef PSREF_TBB_SERIAL_SHIM_H
#define PSREF_TBB_SERIAL_SHIM_H

#include <pthread.h>
#include <stddef.h>
#include <time.h>

#include <utility>

namespace tbb {

template <typename Value>
class blocked_range {
public:
    typedef Value const_iterator;
    blocked_range(Value b, Value e, size_t grain = 1) : m_begin(b), m_end(e), m_grain(grain) {}
    Value begin() const { return m_begin; }
    Value end() const { return m_end; }
    size_t size() const { return size_t(m_end - m_begin); }
    size_t grainsize() const { return m_grain; }
    bool empty() const { return !(m_begin < m_end); }

private:
    Value m_begin, m_end;
    size_t m_grain;
};

class auto_partitioner {};
class simple_partitioner {};

template <typename Range, typename Body>
void parallel_for(const Range& range, const Body& body) {
    if (!range.empty()) body(range);
}
template <typename Range, typename Body, typename Partitioner>
void parallel_for(const Range& range, const Body& body, const Partitioner&) {
    if (!range.empty()) body(range);
}

template <typename T>
class enumerable_thread_specific {
public:
    typedef T& reference;
    typedef const T& const_reference;
    typedef T* iterator;
    typedef const T* const_iterator;

    enumerable_thread_specific() : m_local(0), m_exemplar(0) {}
    explicit enumerable_thread_specific(const T& exemplar) : m_local(0), m_exemplar(new T(exemplar)) {}
    ~enumerable_thread_specific() {
        clear();
        delete m_exemplar;
    }

    reference local() {
        if (!m_local) m_local = m_exemplar ? new T(*m_exemplar) : new T();
        return *m_local;
    }
    void clear() {
        delete m_local;
        m_local = 0;
    }
    size_t size() const { return m_local ? 1 : 0; }
    bool empty() const { return !m_local; }
    iterator begin() { return m_local; }
    iterator end() { return m_local ? m_local + 1 : m_local; }
    const_iterator begin() const { return m_local; }
    const_iterator end() const { return m_local ? m_local + 1 : m_local; }

private:
    enumerable_thread_specific(const enumerable_thread_specific&);
    enumerable_thread_specific& operator=(const enumerable_thread_specific&);
    T* m_local;
    T* m_exemplar;
};

class task_scheduler_observer {
public:
    task_scheduler_observer() : m_observing(false) {}
    virtual ~task_scheduler_observer() {}
    void observe(bool state = true) {
        bool was = m_observing;
        m_observing = state;
        if (state && !was) on_scheduler_entry(false);
    }
    bool is_observing() const { return m_observing; }
    virtual void on_scheduler_entry(bool /*is_worker*/) {}
    virtual void on_scheduler_exit(bool /*is_worker*/) {}

private:
    bool m_observing;
};

class tick_count {
public:
    class interval_t {
    public:
        interval_t() : m_ns(0) {}
        explicit interval_t(long long ns) : m_ns(ns) {}
        double seconds() const { return double(m_ns) * 1e-9; }

    private:
        long long m_ns;
    };
    tick_count() : m_ns(0) {}
    static tick_count now() {
        struct timespec ts;
        clock_gettime(CLOCK_REALTIME, &ts);
        tick_count t;
        t.m_ns = (long long)ts.tv_sec * 1000000000LL + ts.tv_nsec;
        return t;
    }
    friend interval_t operator-(const tick_count& a, const tick_count& b) { return interval_t(a.m_ns - b.m_ns); }

private:
    long long m_ns;
};

class tbb_thread {
public:
    class id {
    public:
        id() : m_id(0) {}
        explicit id(pthread_t t) : m_id(t) {}
        friend bool operator==(const id& a, const id& b) { return a.m_id == b.m_id; }
        friend bool operator!=(const id& a, const id& b) { return a.m_id != b.m_id; }

    private:
        pthread_t m_id;
    };
};

namespace this_tbb_thread {
inline tbb_thread::id get_id() { return tbb_thread::id(pthread_self()); }
}  // namespace this_tbb_thread

}  // namespace tbb

#endif
