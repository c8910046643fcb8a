// prhf_arena.h - the carver of libprhf.so's scratch buffers.  A driver states the layout of a buffer once, as a function
// of a Carver; run over a null base the layout gives the bytes to allocate (used()), run over the buffer's address it
// gives the pointers - so the size asked for is the size carved.  Standard library only, no HIP call: the same code is
// compiled into prhf_api.cpp and into the host test (tests/devtools/arena_host.cpp, tests/test_arena_host.py).

#ifndef PRHF_ARENA_H
#define PRHF_ARENA_H

#include <cstddef>

namespace {

class Carver {
public:
    explicit Carver(void* base) : base_(static_cast<char*>(base)) {}
    // count values of T at the cursor; a null pointer over a null base (the sizing pass)
    template <class T>
    T* take(size_t count) {
        T* p = base_ ? reinterpret_cast<T*>(base_ + used_) : nullptr;
        used_ += count * sizeof(T);
        return p;
    }
    // the cursor, rounded up to a multiple of bytes
    void align(size_t bytes) { used_ = (used_ + bytes - 1) / bytes * bytes; }
    size_t used() const { return used_; }

private:
    char* base_;
    size_t used_ = 0;
};

}  // namespace

#endif  // PRHF_ARENA_H
