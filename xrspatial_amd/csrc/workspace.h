// Layout of a caller-allocated scratch block.  A call's workspace is defined by ONE function, its `carve(base, shape..)`:
// run with a null base it sizes the block (the xrs_*_workspace_bytes / _size entries), run with the block it hands out the
// typed arrays, so the two cannot drift apart.  Plain host C++: nothing of HIP in here.
#pragma once
#include <cstddef>

namespace xrs {

// every part starts on a 256-byte boundary of the block
inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

class Carver {
public:
    explicit Carver(void *base) : base_(static_cast<char *>(base)) {}
    // `count` elements of T at the running offset, which then moves on by up256(count * sizeof(T)); a count of 0 takes no
    // bytes and returns the address of the next part.  A null base (the sizing pass) gives null pointers.
    template <typename T>
    T *take(size_t count) { return take_bytes<T>(up256(count * sizeof(T))); }
    // exactly `bytes` bytes, NOT rounded: for the parts that are not up256(count * sizeof(T)) -- a 256-byte word for a
    // single counter, up256(n) + 256 in front of a hipCUB block.  The caller passes a multiple of 256.
    template <typename T = void>
    T *take_bytes(size_t bytes) {
        T *p = base_ ? reinterpret_cast<T *>(base_ + at_) : nullptr;
        at_ += bytes;
        return p;
    }
    size_t at() const { return at_; }          // bytes handed out so far: the offset of the next part, at the end the total

private:
    char *base_;
    size_t at_ = 0;
};

}  // namespace xrs
