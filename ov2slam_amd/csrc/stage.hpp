// stage.hpp -- the layout half of the staging rule of the stand-alone calls (host conventions): the sections of one call
// lie in ONE scratch block, inputs first, at the same offsets on the device and in the pinned host block.  Here: the two roundings
// every layout uses and the cursor that hands out section offsets.  Plain C++ (no HIP types, no context): the layout headers and the
// .hip files include it, tests/test_stage_layout.py compiles it alone with g++.  The round trip itself is `Stage` in common.hpp.
#pragma once
#include <stddef.h>

static inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }
static inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// Sections of a block in the order of the take() calls: take(bytes) returns where the section starts and moves `off` to the next
// multiple of `align` (a power of two, given once per block: 16, 256 or 8; 1 packs) behind it.  After the last take `off` is the
// block's total.  The numbers are those of the chain o_k = al(o_{k-1} + s_{k-1}), total = al(o_last + s_last); a section of 0 bytes
// takes no room and shares its start with the next one.
struct StageCursor {
    size_t align, off = 0;
    explicit StageCursor(size_t align_) : align(align_) {}
    size_t take(size_t bytes)
    {
        const size_t o = off;
        off = (off + bytes + align - 1) & ~(align - 1);
        return o;
    }
};
