// The one way arrays are carved out of a device scratch buffer. Host-only: no HIP headers, usable from g++.
#pragma once

#include <algorithm>
#include <cstddef>

namespace eacham {

struct Bump {  // carves 256-byte aligned arrays out of a scratch buffer (base == nullptr: sizes only)
    char* base;
    size_t off = 0;
    explicit Bump(void* b) : base((char*)b) {}
    template <class T>
    T* take(size_t n) {
        T* p = base ? (T*)(base + off) : nullptr;
        off += (std::max<size_t>(n, 1) * sizeof(T) + 255) & ~(size_t)255;
        return p;
    }
};

}  // namespace eacham
