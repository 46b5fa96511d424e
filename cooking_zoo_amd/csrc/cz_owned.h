// cz_owned.h -- one move-only owner of a raw handle (a device or pinned pointer, a stream, an event, a graph): released exactly once, by
// the function it is bound to, when the owner dies or is given something else.  Converts to the raw type implicitly, so code that
// only uses the resource reads as if the field were raw.  No HIP header: the aliases that bind it to hipFree and the like stand beside
// the handle (cz_api.hip), and tests/test_owned_host.py builds this file alone for the CPU.
#pragma once
#include <utility>

namespace cz {

template <class T, auto Release>
class __attribute__((visibility("hidden"))) Owned {      // (no instantiation is exported from a shared library)
    T raw_ = T();

public:
    Owned() = default;
    explicit Owned(T raw) : raw_(raw) {}
    Owned(Owned &&o) noexcept : raw_(o.release()) {}
    Owned &operator=(Owned &&o) noexcept {
        if (this != &o) reset(o.release());
        return *this;
    }
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    ~Owned() { reset(); }

    T get() const { return raw_; }
    operator T() const { return raw_; }
    // releases what is held, then holds `raw`
    void reset(T raw = T()) {
        if (raw_) (void)Release(raw_);
        raw_ = raw;
    }
    // hands the resource to the caller without releasing it
    T release() { return std::exchange(raw_, T()); }
    // for calls that create through an out-parameter (hipMalloc(x.out(), bytes)): releases what is held, then exposes the empty slot
    T *out() {
        reset();
        return &raw_;
    }
};

}  // namespace cz
