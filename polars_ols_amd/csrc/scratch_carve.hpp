// scratch_carve.hpp -- one work buffer cut into regions, each declared ONCE: the sum that sizes the buffer and the offset of every
// pointer into it come from the same list, so a region cannot be in one and missing from the other.  Plain C++ (no HIP): the host
// entries use it, tests/carve_check.cpp checks it on the CPU.  Two phases:
//     Carve cv;
//     cv.add(a.gram_part, sizeof(double) * items * stride);      // a typed slot and its bytes (rounded up to 256 here; a pad the
//     cv.add(a.state, sizeof(double) * G * n + 8);               //  kernels rely on stays inside the count the entry passes)
//     ... ensure_scratch(ctx, Work::X, cv.total(), &base) ...    // ONE allocation of the total
//     cv.place(base);                                            // every slot = base + its offset, in the order of the adds
// A region of 0 bytes is absent: it takes no room and its slot becomes nullptr, or what `instead` points to once the present regions
// are placed (fold_gram = fold_part when nothing is split).  keep() is the other convention: the region KEEPS its room whether or not
// it is wanted, so that nothing behind it moves; a wanted slot is placed whatever its size (an empty frame's columns still have an
// address) and an unwanted one becomes nullptr (the staged outputs of a host batch).  gap() is such room without a slot: a fixed pad.  A region that lays its inside out itself is a
// char slot; a table that repeats (once per id column) is a loop around the adds; a run of n equal columns is ONE region of n strides
// and column(base, stride, j) its j-th column -- the only pointer arithmetic left on a buffer's inside.
#pragma once

#include <cassert>
#include <cstddef>

namespace pols {

// (hidden: a helper of the host entries, no part of what the shared library exports)
class __attribute__((visibility("hidden"))) Carve {
public:
    static constexpr int CAP = 32;
    static size_t round(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

    template <typename T> void add(T *&slot, size_t bytes, T **instead = nullptr) { region(slot, bytes, bytes > 0, instead); }
    template <typename T> void keep(T *&slot, size_t bytes, bool wanted = true) { region(slot, bytes, wanted, (T **)nullptr); }
    void gap(size_t bytes) { total_ += round(bytes); }
    size_t total() const { return total_; }
    void place(void *base) const {
        for (int i = 0; i < n_; ++i)
            if (r_[i].present) r_[i].set(r_[i].slot, static_cast<char *>(base) + r_[i].offset, nullptr);
        for (int i = 0; i < n_; ++i)
            if (!r_[i].present) r_[i].set(r_[i].slot, nullptr, r_[i].instead);
    }

private:
    struct Region {
        void *slot, *instead;
        size_t offset;
        bool present;
        void (*set)(void *slot, void *p, void *from);
    };
    template <typename T> void region(T *&slot, size_t bytes, bool present, T **instead) {
        assert(n_ < CAP);
        r_[n_++] = Region{&slot, instead, total_, present, [](void *s, void *p, void *from) {
                              *static_cast<T **>(s) = from ? *static_cast<T **>(from) : static_cast<T *>(p);
                          }};
        total_ += round(bytes);
    }
    Region r_[CAP];
    int n_ = 0;
    size_t total_ = 0;
};

// the j-th of a region's equal columns, `stride` bytes apart
template <typename T> T *column(T *base, size_t stride, size_t j) { return (T *)((const char *)base + stride * j); }

}  // namespace pols
