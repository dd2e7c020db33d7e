// io_layout.hpp — where the arrays of one host-pointer call lie in the staging buffer (IoStage, context.hpp). Plain C++ without
// HIP: tests/cpp/io_layout_driver.cpp compiles it with g++ (as tests/cpp/plan_driver.cpp does ba_plan.hpp).
//
// Sizes and roles in; offsets, the mirror cut and the total out. Whatever the order of the declarations: the results, then the
// inputs (each side one contiguous run, so each travels as one span of the pinned mirror), then what never passes through the
// mirror. Every array starts on a 256-byte boundary; an array of no bytes takes no room.
#pragma once

#include <cstddef>

namespace eacham {

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

enum IoRole { IO_OUT = 0, IO_IN = 1, IO_DEV = 2 };

struct IoLayout {
    static constexpr int MAX_ARRAYS = 32;
    int n = 0;
    bool overflow = false;   // a declaration beyond MAX_ARRAYS: the call is refused (IoStage::upload), never laid out short
    int role[MAX_ARRAYS];
    size_t bytes[MAX_ARRAYS], off[MAX_ARRAYS];
    size_t cut = 0;     // first byte of the device-only group = what the pinned mirror has to cover
    size_t total = 0;

    int add(int r, size_t b) {
        if (n == MAX_ARRAYS) { overflow = true; return 0; }
        role[n] = r, bytes[n] = b, off[n] = 0;
        return n++;
    }
    void place() {
        size_t o = 0;
        for (int r = IO_OUT; r <= IO_DEV; ++r) {
            if (r == IO_DEV) cut = o;
            for (int k = 0; k < n; ++k)
                if (role[k] == r) { off[k] = o; o = align256(o + bytes[k]); }
        }
        total = o;
    }
};

}  // namespace eacham
