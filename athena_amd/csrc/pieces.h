// One allocation cut into pieces: list the arrays of a call with add(), ask bytes() of the allocator, place() hands every array its
// pointer.  Every piece starts on a 256-byte boundary of the base.  No HIP in here: Scratch::carve of common.h and the sampler's
// GrowBuffer supply the base, and a plain host program can test the arithmetic.
// The caller's contract: a piece of 0 elements takes no room and points where the next one begins (base + bytes() for the last),
// so it has NO element of its own -- unlike Scratch::get, which hands out at least one.  Whoever may write element 0 of an array
// that can be empty (a memset of max(n, 1) words, a kernel's slot [n]) adds it with max(n, 1), as csr_from_edges_core does with
// its loop flags; every other core returns before its carve when a size is 0.  An array that is not added keeps the pointer it had.
#pragma once
#include <stddef.h>
#include <string.h>

#include <vector>

namespace amp {

struct Pieces {
    Pieces() { slots.reserve(16); }                                   // the longest list has 15: one host allocation a call
    template <typename T> void add(T **p, size_t count)
    {
        slots.push_back(Slot{p, total});
        total += (count * sizeof(T) + 255) & ~(size_t)255;
    }
    size_t bytes() const { return total; }
    void place(char *base)
    {
        for (const Slot &s : slots) {
            char *at = base + s.at;
            memcpy(s.p, &at, sizeof(at));                             // *p = (T *)at, whatever T was
        }
    }

private:
    struct Slot {
        void *p;                                                      // the T ** of add()
        size_t at;
    };
    std::vector<Slot> slots;
    size_t total = 0;
};

} // namespace amp
