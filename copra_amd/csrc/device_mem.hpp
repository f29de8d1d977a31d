// device_mem.hpp -- ownership of device and pinned memory by type.  Host only; no HIP header: the allocator is a policy `Mem` with
//   static int  alloc(void** p, size_t bytes);                      0 on success, else its error code (*p untouched or null)
//   static void release(void* p);
//   static int  copy_in(void* dst, const void* src, size_t bytes);  (DevBag only) host -> block
// The HIP policies are in engine.hpp; tests/cpp/test_device_mem.cpp has a counting one.
// A member that OWNS memory is a DevBuf / DevBag; a raw pointer next to it is borrowed or a view.  All-or-none groups need no helper:
// allocate into locals and move them into the members once every one has succeeded -- a failed attempt then leaves the members as they were.
#pragma once
#include <cstddef>
#include <memory>
#include <utility>
#include <vector>

// Move-only owner of `count` elements.  Reads as the T* it holds (h->d_x + i, P.ws = h->d_x, if (!h->d_x)); there is no way to take the
// pointer out of it and no operator&.
template <class T, class Mem>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr, o.n_ = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        if (this != std::addressof(o)) {
            reset();
            p_ = o.p_, n_ = o.n_;
            o.p_ = nullptr, o.n_ = 0;
        }
        return *this;
    }
    ~DevBuf() { reset(); }

    // a fresh block of `count` elements; what was held is released first, and a failed attempt leaves the buffer empty
    int alloc(size_t count)
    {
        reset();
        void* p = nullptr;
        const int rc = Mem::alloc(&p, count * sizeof(T));
        if (rc != 0) return rc;
        p_ = static_cast<T*>(p), n_ = count;
        return 0;
    }
    // ... only when `count` exceeds what is held
    int grow(size_t count) { return (p_ && count <= n_) ? 0 : alloc(count); }
    void reset()
    {
        if (p_) Mem::release(p_);
        p_ = nullptr, n_ = 0;
    }
    T* get() const { return p_; }
    size_t count() const { return n_; }
    operator T*() const { return p_; }
    explicit operator bool() const { return p_ != nullptr; }
    void operator&() const = delete; // ((void**)&member handed to an allocator or a kernel-argument list would compile and be wrong)

private:
    T* p_ = nullptr;
    size_t n_ = 0;
};

// Move-only list of untyped blocks, all released with it.  The first error of any add() stays in error(); add() after an error still
// returns null or a block, so a caller checks once, after the last.
template <class Mem>
class DevBag {
public:
    DevBag() = default;
    DevBag(const DevBag&) = delete;
    DevBag& operator=(const DevBag&) = delete;
    DevBag(DevBag&& o) noexcept : blocks_(std::move(o.blocks_)), err_(o.err_) { o.blocks_.clear(), o.err_ = 0; }
    DevBag& operator=(DevBag&& o) noexcept
    {
        if (this != &o) {
            reset();
            blocks_ = std::move(o.blocks_), err_ = o.err_;
            o.blocks_.clear(), o.err_ = 0;
        }
        return *this;
    }
    ~DevBag() { reset(); }

    // `count` elements of T (a block of one element when count is 0), filled from *src when given
    template <class T>
    T* add(size_t count, const std::vector<T>* src = nullptr)
    {
        void* p = nullptr;
        int rc = Mem::alloc(&p, (count ? count : 1) * sizeof(T));
        if (rc != 0) p = nullptr;
        else blocks_.push_back(p);
        if (rc == 0 && src && !src->empty()) rc = Mem::copy_in(p, src->data(), src->size() * sizeof(T));
        if (rc != 0 && err_ == 0) err_ = rc;
        return static_cast<T*>(p);
    }
    int error() const { return err_; }
    size_t size() const { return blocks_.size(); }
    void reset()
    {
        for (void* p : blocks_) Mem::release(p);
        blocks_.clear();
        err_ = 0;
    }

private:
    std::vector<void*> blocks_;
    int err_ = 0;
};
