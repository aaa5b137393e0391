"""Static instruction counts of the two hot kernels, from a device-only compile for gfx950 (the compile line of
tests/test_lk3_resources.py).  No GPU needed; skipped without hipcc.  `python tests/test_hot_kernel_isa.py` prints the figures;
OV2_ISA_ROOT=<another checkout> takes them from that tree (how the parent's were taken).

k_fb_klt3 (lk3.hip): the rounding constant 2^15 of the derivative taps rides in a scalar register of the three-address
v_dot2_i32_i16, so no `v_mov_b32 vN, 0x8000` is left, and the kernel's static VALU count stays below the parent's.

k_clahe_apply_pyr<false, *> (clahe.hip): the fast six-row group exists once per kind of strip (middle of the image, image
edge, either).  A row here is what stands between two consecutive buffer_store_dword stores to the lane's own column: five
rows per group.  No row reloads or saves a spilled scalar (v_readlane_b32 / v_writelane_b32 of the spill register; the two
v_readlane_b32 that fetch the row's vertical weights read another register and count as VALU).  VALU bounds, from the
expectation of 57 per row without its share of the level-1 emits (22 VALU per emit at the parent, one emit per two rows, 11 per
row): the scheduler moves an emit's instructions across a row store, so a single row may hold a whole emit, 57 + 22, and a
group's mean is bound by 57 + 11; the middle-strip group also drops the two v_cndmask of the edge columns, 55 + 11.

                                              parent 3876083                  this commit
  k_fb_klt3 VALU, static                      2369                            2244
  k_fb_klt3 v_mov_b32 .., 0x8000              108 (54 per build instance)     0
  <false, true>  rows (VALU)                  76 61 86 60 82, mean 73.0       55 65 57 65 56 | 59 69 61 69 60 | 65 72 66 72 64
  <false, true>  spill lane moves in them     7                               0
  <false, false> rows (VALU)                  76 65 87 63 82, mean 74.6       the same as <false, true>
  <false, false> spill lane moves in them     15                              0
"""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.environ.get("OV2_ISA_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))     # (another checkout: the parent's figures)
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")

KLT3_VALU_PARENT = 2369         # static VALU instructions of k_fb_klt3 at the parent commit 3876083
ROW_VALU = 57                   # a fast-path row with the v_readlane form of the vertical weights, without its emit share
EMIT_VALU = 22                  # a level-1 emit at the parent (rows with one: 76, 86, 82; without: 61, 60), one per two rows
_cache = {}


def kernels(name):
    """{kernel symbol: [instruction lines]} of ov2slam_amd/csrc/<name>.hip, compiled once per session."""
    if name not in _cache:
        import tempfile
        src = os.path.join(ROOT, "ov2slam_amd", "csrc", name + ".hip")
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, name + ".s")
            subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                            "--cuda-device-only", "-S", src, "-o", out], check=True, capture_output=True)
            txt = open(out).read()
        res = {}
        for m in re.finditer(r"^(\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", txt, re.S | re.M):
            body = [ln.split(";")[0].strip() for ln in m.group(2).splitlines()]
            res[m.group(1)] = [ln for ln in body if ln and (ln.endswith(":") or not ln.startswith("."))]     # instructions and labels
        _cache[name] = res
    return _cache[name]


def one(name, part):
    ks = [k for k in kernels(name) if part in k]
    assert len(ks) == 1, ks
    return kernels(name)[ks[0]]


def is_valu(ins):
    return ins.startswith("v_")


def spill_register(body):
    """The VGPR that holds spilled scalars: the destination of the v_writelane_b32 instructions."""
    regs = {re.split(r"[ ,]+", i)[1] for i in body if i.startswith("v_writelane_b32")}
    return regs


def fast_rows(body):
    """The fast groups of a strip kernel: runs without a loop (no backward branch or its target, no s_branch, no barrier; the
    forward branches around an edge strip's border stores stay inside) that hold at least six level-0 row stores to the
    lane's own column.  Returns, per group, the list of rows; a row is the instruction list between two consecutive row stores
    (the first of a row's stores)."""
    where = {ins[:-1]: n for n, ins in enumerate(body) if ins.endswith(":")}
    cuts = set()
    for n, ins in enumerate(body):
        if ins.startswith(("s_branch", "s_barrier", "s_setpc")):
            cuts.add(n)
        elif ins.startswith("s_cbranch"):
            t = where.get(ins.split()[-1])
            if t is None or t < n:
                cuts.add(n); cuts.add(t if t is not None else n)
            elif t - n > 150:                   # a branch over a whole group (the groups of the three strip kinds lie in a row)
                cuts.add(n)
    groups, cur = [], []
    for n, ins in enumerate(body):
        if n in cuts:
            groups.append(cur); cur = []
        if not ins.endswith(":"):
            cur.append(ins)
    groups.append(cur)
    out = []
    for g in groups:
        stores = [(n, ins.split(",")[1].strip()) for n, ins in enumerate(g) if ins.startswith("buffer_store_dword")]
        idx = [n for n, vaddr in stores if vaddr == stores[0][1]]       # the lane's own column, not its border column
        if len(idx) >= 6:
            out.append([g[a:b] for a, b in zip(idx[:-1], idx[1:])])
    return out


def row_report(body):
    """Per fast group, per row: (VALU instructions, lane moves of the spill register)."""
    spill = spill_register(body)
    rep = []
    for rows in fast_rows(body):
        grp = []
        for r in rows:
            valu = sum(is_valu(i) for i in r)
            lanes = [i for i in r if i.startswith(("v_readlane_b32", "v_writelane_b32")) and
                     any(re.search(r"\b%s\b" % s, i) for s in spill)]
            grp.append((valu, len(lanes)))
        rep.append(grp)
    return rep


@needs_hipcc
def test_klt3_has_no_rounding_constant_moves():
    body = one("lk3", "k_fb_klt3")
    movs = [i for i in body if re.match(r"v_mov_b32\S*\s+v\d+, 0x8000$", i)]
    assert not movs, movs


@needs_hipcc
def test_klt3_static_valu_below_parent():
    n = sum(is_valu(i) for i in one("lk3", "k_fb_klt3"))
    print("k_fb_klt3 static VALU:", n, "parent:", KLT3_VALU_PARENT)
    assert n < KLT3_VALU_PARENT, n


@needs_hipcc
@pytest.mark.parametrize("inst", ["ILb0ELb1EE", "ILb0ELb0EE"], ids=["fused", "plain"])
def test_strip_fast_rows(inst):
    rep = row_report(one("clahe", "k_clahe_apply_pyr" + inst))
    print(inst, "fast-path rows (VALU, spill lane moves):", rep)
    assert len(rep) == 3 and all(len(g) == 5 for g in rep), rep         # one six-row group per kind of strip
    assert all(l == 0 for g in rep for _, l in g), rep
    assert max(v for g in rep for v, _ in g) <= ROW_VALU + EMIT_VALU, rep
    means = [sum(v for v, _ in g) / len(g) for g in rep]
    assert max(means) <= ROW_VALU + EMIT_VALU / 2, means
    assert min(means) <= ROW_VALU - 2 + EMIT_VALU / 2, means              # the middle strips' group


if __name__ == "__main__":
    body = one("lk3", "k_fb_klt3")
    print("k_fb_klt3 VALU", sum(is_valu(i) for i in body), "v_mov 0x8000",
          sum(bool(re.match(r"v_mov_b32\S*\s+v\d+, 0x8000$", i)) for i in body))
    for inst in sys.argv[1:] or ["ILb0ELb1EE", "ILb0ELb0EE", "ILb1ELb1EE", "ILb1ELb0EE"]:
        print(inst, row_report(one("clahe", "k_clahe_apply_pyr" + inst)))
