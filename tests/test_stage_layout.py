"""The layout half of the stand-alone calls' staging rule (ov2slam_amd/csrc/stage.hpp): the two roundings and the section cursor.  The
header is plain C++; a small program compiled here with g++ (like tests/test_lockstep_layout.py does for its header) prints the
cursor's offsets and totals for lists of section sizes at every alignment in use, and every line is compared with the chain the host
drivers used to write by hand, o_k = al(o_{k-1} + s_{k-1}), total = al(o_last + s_last), restated below."""
import functools
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALIGNS = (1, 8, 16, 256)
# a zero-size section first, in the middle and last; 1, 15, 16, 17 bytes around the 16-byte boundary; nothing but empty sections; one
# section; a list like knn's at a count that ends its byte-sized section off a boundary; a total beyond 2^32 (an int in the cursor shows)
SIZES = (
    (0, 1, 15, 0, 16, 17, 0),
    (1, 15, 16, 17),
    (17, 16, 15, 1),
    (0, 0, 0),
    (255,),
    (16 * 3, 32 * 17, 32 * 23, 8 * 17, 8 * 17, 17),
    (1 << 31, 0, (1 << 31) + 1, 17, 1 << 32),
)
UPS = (0, 1, 15, 16, 17, 255, 256, 257, (1 << 32) + 1)

SRC = r"""
#include <cstdio>
#include <vector>
#include "stage.hpp"
int main()
{
    const size_t aligns[] = {ALIGNS};
    const std::vector<std::vector<size_t>> lists = {SIZES};
    for (size_t a : aligns)
        for (size_t k = 0; k < lists.size(); k++) {
            StageCursor c(a);
            printf("cursor %zu %zu", a, k);
            for (size_t s : lists[k]) printf(" %zu", c.take(s));
            printf(" %zu\n", c.off);
        }
    const size_t ups[] = {UPS};
    for (size_t v : ups) printf("up %zu %zu %zu\n", v, up16(v), up256(v));
    return 0;
}
"""


def _ull(v):
    return "%dull" % v


@functools.lru_cache(maxsize=None)
def layout():
    """{(align, list index): (offsets..., total)} and [(v, up16(v), up256(v))] as the program prints them"""
    src = SRC.replace("ALIGNS", ", ".join(_ull(a) for a in ALIGNS)).replace("UPS", ", ".join(_ull(v) for v in UPS))
    src = src.replace("SIZES", ", ".join("{%s}" % ", ".join(_ull(s) for s in row) for row in SIZES))
    with tempfile.TemporaryDirectory() as tmp:
        cpp, exe = os.path.join(tmp, "t.cpp"), os.path.join(tmp, "t")
        with open(cpp, "w") as f:
            f.write(src)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "ov2slam_amd", "csrc"), cpp, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout
    cursor, ups = {}, []
    for line in out.splitlines():
        key, *vals = line.split()
        vals = tuple(int(v) for v in vals)
        if key == "cursor":
            cursor[vals[:2]] = vals[2:]
        else:
            ups.append(vals)
    return cursor, ups


def al(v, a):
    return (v + a - 1) & ~(a - 1)


def chain(sizes, a):
    """the hand-written form: every offset is the rounded end of the section before it, the total the rounded end of the last"""
    offsets = [0]
    for s in sizes[:-1]:
        offsets.append(al(offsets[-1] + s, a))
    return tuple(offsets) + (al(offsets[-1] + sizes[-1], a),)


def test_rounding():
    _, ups = layout()
    assert [u[0] for u in ups] == list(UPS)
    for v, a, b in ups:
        assert (a, b) == (al(v, 16), al(v, 256)) and a % 16 == 0 and b % 256 == 0 and 0 <= a - v < 16 and 0 <= b - v < 256
    assert ups[-1][0] > 1 << 32 and ups[-1][1] == (1 << 32) + 16 and ups[-1][2] == (1 << 32) + 256


def test_cursor_is_the_chain():
    cursor, _ = layout()
    assert set(cursor) == {(a, k) for a in ALIGNS for k in range(len(SIZES))}
    for (a, k), got in cursor.items():
        assert got == chain(SIZES[k], a), (a, SIZES[k])


def test_cursor_sections():
    """what a driver relies on: ascending from 0, every start and the total on the block's alignment, no section reaching into the
    next, no more than align - 1 bytes of padding behind a section, an empty section sharing its start with its successor"""
    cursor, _ = layout()
    for (a, k), got in cursor.items():
        sizes, offsets, total = SIZES[k], list(got[:-1]), got[-1]
        assert offsets[0] == 0 and offsets == sorted(offsets)
        for o, s, e in zip(offsets, sizes, offsets[1:] + [total]):
            assert o % a == 0 and e % a == 0 and 0 <= e - (o + s) < a, (a, sizes, got)
            assert s != 0 or e == o
        if a == 1:
            assert total == sum(sizes)                                  # packed
    assert cursor[16, len(SIZES) - 1][-1] > 1 << 32
