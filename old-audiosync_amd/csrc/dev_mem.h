// csrc/dev_mem.h — who owns device memory: a set of allocations over an ops pair (asx_api.hip binds it to hipMalloc / hipFree,
// tests/c/dev_mem_test.cpp to malloc / free with a failing k-th take).  No HIP in it.
#pragma once
#include <cstddef>
#include <utility>
#include <vector>

struct AsxMemOps {
    int (*take)(void **out, size_t bytes); // 0, or -1
    void (*give)(void *p);
};

// Gives back what it holds when it dies or is cleared; moved, never copied.
class AsxMemSet {
    std::vector<void *> held_;
    size_t bytes_ = 0;
public:
    const AsxMemOps ops;
    explicit AsxMemSet(AsxMemOps o) : ops(o) {}
    AsxMemSet(AsxMemSet &&o) : ops(o.ops) { swap(o); }
    ~AsxMemSet() { clear(); }
    void clear() { for (void *p : held_) ops.give(p); held_.clear(); bytes_ = 0; }
    template <typename T> int take(T **out, size_t count) // count elements of T; 0: one element, so that every piece has an address
    {
        void *p = nullptr;
        const size_t bytes = (count ? count : 1) * sizeof(T);
        if (ops.take(&p, bytes) != 0) return -1;
        held_.push_back(p);
        bytes_ += bytes;
        *out = static_cast<T *>(p);
        return 0;
    }
    size_t bytes() const { return bytes_; }
    void swap(AsxMemSet &o) { held_.swap(o.held_); std::swap(bytes_, o.bytes_); }
    void adopt(AsxMemSet &o) { held_.insert(held_.end(), o.held_.begin(), o.held_.end()); bytes_ += o.bytes_; o.held_.clear(); o.bytes_ = 0; }
};

// A set of pointers (a struct P) that exists whole or not at all: fill(set, pointers) takes the pieces from a local set into a copy
// of dst.  When it returns 0 the owner adopts them and dst is assigned; else all of them go back at once and neither has changed.
template <typename P, typename F> int asx_mem_whole(AsxMemSet &owner, P &dst, F fill)
{
    AsxMemSet local(owner.ops);
    P t = dst;
    if (fill(local, t) != 0) return -1;
    owner.adopt(local);
    dst = t;
    return 0;
}
