// device_mem.hpp -- ownership of device and pinned memory by type.  Host only; no HIP header: the allocator is a policy `Mem` with
//   static int  alloc(void** p, size_t bytes);                      0 on success, else its error code (*p untouched or null)
//   static void release(void* p);
//   static int  copy_in(void* dst, const void* src, size_t bytes);  (DevBag only) host -> block
// The HIP policies are in engine.hpp; tests/cpp/test_device_mem.cpp has a counting one.
// A member that OWNS memory is a DevBuf / DevBag; a raw pointer next to it is borrowed or a view.  An array that a setter takes either on
// the device (borrowed) or from the host (copied) is ONE member, a DevArg: the view in force and the copy behind it.  All-or-none groups need no helper:
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

// An input array that is the caller's device array or the library's copy of a host array: the `const T*` in force (null: unset) and the
// copy, which outlives a borrow() and an unset() "for the next time".  Reads as the view (if (x), Q.C = h->obs_C).  Nothing here waits for
// the device -- Mem has no stream: whoever calls copy_in() has waited for what may still read the old copy.
template <class T, class Mem>
class DevArg {
public:
    DevArg() = default;
    DevArg(const DevArg&) = delete;
    DevArg& operator=(const DevArg&) = delete;
    DevArg(DevArg&& o) noexcept : view_(o.view_), copy_(std::move(o.copy_)) { o.view_ = nullptr; }
    DevArg& operator=(DevArg&& o) noexcept // (a view of o's copy follows it: a block's address does not change with its owner)
    {
        if (this != std::addressof(o)) {
            view_ = o.view_, o.view_ = nullptr;
            copy_ = std::move(o.copy_);
        }
        return *this;
    }

    // the caller's device array; the copy is kept
    void borrow(const T* device_ptr) { view_ = device_ptr; }
    // the library's copy of `count` host elements (a block of one element when count is 0), grown only when it is too small.  The view is
    // null from the first step on and stays null when the allocation or the copy fails, whose error code is returned
    int copy_in(const T* host, size_t count)
    {
        view_ = nullptr;
        int rc = copy_.grow(count ? count : 1);
        if (rc == 0 && count) rc = Mem::copy_in(copy_.get(), host, count * sizeof(T));
        if (rc != 0) return rc;
        view_ = copy_.get();
        return 0;
    }
    void unset() { view_ = nullptr; } // the copy is kept
    void reset() // ... and here it goes
    {
        view_ = nullptr;
        copy_.reset();
    }
    const T* get() const { return view_; }
    const DevBuf<T, Mem>& copy() const { return copy_; }
    operator const T*() const { return view_; }
    explicit operator bool() const { return view_ != nullptr; }

private:
    const T* view_ = nullptr;
    DevBuf<T, Mem> copy_;
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
