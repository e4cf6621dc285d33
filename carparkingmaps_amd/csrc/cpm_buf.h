// cpm_buf.h -- the owner of one device or pinned-host allocation of the context (host only: no HIP header is included here, the
// allocator is a policy; cpm_api.hip names the two it uses, tests/buf_host.cc a counting one).
#pragma once

#include <cstddef>

namespace cpm {

// A: struct { using error = ...; static constexpr error ok = ...; static error alloc(void **p, size_t bytes); static void free(void *p); }
template <typename T, typename A>
class Buf {
public:
    T *p = nullptr;
    size_t cap = 0;  // elements p holds room for (0: nothing is allocated)

    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    ~Buf() { release(); }

    bool fits(size_t n) const { return p && cap >= n; }

    // Room for n elements (at least one, so the pointer of a reserved buffer is never null).  Grow-only, and the contents are NOT
    // kept across a grow: the old allocation is freed first.  A failed allocation leaves {nullptr, 0}: the next call tries again.
    typename A::error reserve(size_t n)
    {
        if (fits(n)) return A::ok;
        release();
        const size_t m = n > 0 ? n : 1;
        void *q = nullptr;
        const typename A::error e = A::alloc(&q, sizeof(T) * m);
        if (e != A::ok) return e;
        p = static_cast<T *>(q);
        cap = m;
        return A::ok;
    }

    void release()
    {
        if (p) A::free(p);
        p = nullptr;
        cap = 0;
    }

    // two owners trade their allocations (the ping-pong of the car state): neither is ever pointed at memory it does not own
    void swap(Buf &o)
    {
        T *const tp = p;
        const size_t tc = cap;
        p = o.p;
        cap = o.cap;
        o.p = tp;
        o.cap = tc;
    }

    T *get() const { return p; }
    operator T *() const { return p; }
};

}  // namespace cpm
