"""The layouts of the lock-step tracker's host-visible blocks (ov2slam_amd/csrc/trackb_layout.hpp): the point block, the map block, the
pose block, the epipolar I/O block and the filter's index block.  The header is plain C++; a small program compiled here with g++ (like
tests/test_detect_plan.py does for its header) prints every offset and total, and every line is compared with the restatement of the
formulas written below.  Per block: the documented order, the 256-byte starts, no section reaching into the next, and the upload
prefix ending where the download suffix begins."""
import functools
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# smallest; the GPU tests' shape; a node's shard; the benchmark's shape; both limits (totals beyond 32 bits: an int in the arithmetic shows)
CASES = ((1, 1), (3, 40), (11, 308), (4096, 308), (65535, 2048))
IMAGES = ((1, 1), (376, 240), (752, 480), (1241, 376))
POSE_OUT, EPIF_OUT, KF_HDR = 168, 304, 120

SRC = r"""
#include <cstdio>
#include "trackb_layout.hpp"
int main()
{
    printf("const %d %d %d\n", BT_POSE_OUT_BYTES, BT_EPIF_OUT_BYTES, BT_KF_HDR_BYTES);
    const int cases[][2] = {CASES};
    for (auto &c : cases) {
        const BtPointLayout p = bt_point_layout(c[0], c[1]);
        printf("point %d %d %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", c[0], c[1], p.o_n, p.o_kps, p.o_pri, p.o_flg, p.in_bytes, p.o_out, p.o_st,
               p.o_unpx, p.o_bv, p.blk_bytes);
        const BtMapLayout m = bt_map_layout(c[0], c[1]);
        printf("map %d %d %zu %zu %zu %zu %zu\n", c[0], c[1], m.m_it, m.m_T, m.m_w, m.m_3d, m.map_bytes);
        const BtPoseLayout q = bt_pose_layout(c[0], c[1]);
        printf("pose %d %d %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", c[0], c[1], q.q_T, q.q_seed, q.q_fl, q.q_sc, q.q_in, q.q_out, q.q_ms, q.q_rm,
               q.pose_bytes);
        const BtEpiLayout e = bt_epi_layout(c[0], c[1]);
        printf("epi %d %d %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", c[0], c[1], e.e_lm, e.e_nk, e.e_sd, e.e_in, e.e_out, e.e_nc, e.e_rm, e.e_er,
               e.e_pc, e.epi_bytes);
        printf("fx %d %d %zu %zu %zu\n", c[0], c[1], e.x_slot, e.x_rank, e.fx_bytes);
        printf("det %d %d %zu\n", c[0], c[1], bt_det_in_bytes(c[0], c[1]));
    }
    const int images[][2] = {IMAGES};
    for (auto &i : images) printf("img %d %d %zu %zu\n", i[0], i[1], bt_img_pitch(i[0]), bt_img_bytes(i[0], i[1]));
    const size_t ups[] = {0, 1, 15, 16, 17, 255, 256, 257, ((size_t)1 << 32) + 1};
    for (size_t v : ups) printf("up %zu %zu %zu\n", v, up16(v), up256(v));
    return 0;
}
"""


def _csv(rows):
    return ", ".join("{%s}" % ", ".join(str(v) for v in r) for r in rows)


@functools.lru_cache(maxsize=None)
def layout():
    """every line the program prints, grouped by its first word; a (batch, n_max) line as {(batch, n_max): values}"""
    src = SRC.replace("CASES", _csv(CASES)).replace("IMAGES", _csv(IMAGES))
    with tempfile.TemporaryDirectory() as tmp:
        cpp, exe = os.path.join(tmp, "t.cpp"), os.path.join(tmp, "t")
        with open(cpp, "w") as f:
            f.write(src)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "ov2slam_amd", "csrc"), cpp, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout
    rows = {}
    for line in out.splitlines():
        key, *vals = line.split()
        vals = tuple(int(v) for v in vals)
        if key in ("const", "up"):
            rows.setdefault(key, []).append(vals)
        else:
            rows.setdefault(key, {})[vals[:2]] = vals[2:]
    return rows


def up16(v):
    return (v + 15) & ~15


def up256(v):
    return (v + 255) & ~255


def _sections_ok(offsets, sizes, total, aligned):
    """ascending from 0, inside [0, total], no section reaching into the next; `aligned`: which start on a 256-byte boundary"""
    ends = offsets[1:] + [total]
    for i, (o, n, e) in enumerate(zip(offsets, sizes, ends)):
        assert o + n <= e, (i, offsets, sizes, total)
        assert not aligned[i] or o % 256 == 0, (i, offsets)
    assert offsets == sorted(offsets) and offsets[0] == 0


def test_constants_and_rounding():
    assert layout()["const"] == [(POSE_OUT, EPIF_OUT, KF_HDR)]
    for v, a, b in layout()["up"]:
        assert (a, b) == (up16(v), up256(v)) and a % 16 == 0 and b % 256 == 0 and 0 <= a - v < 16 and 0 <= b - v < 256
    assert len(layout()["up"]) == 9 and layout()["up"][-1][0] > 1 << 32
    assert set(layout()["point"]) == set(CASES)
    for (w, h), (pitch, nbytes) in layout()["img"].items():
        assert pitch == up16(w) and nbytes == up256(pitch * h) and pitch >= w
    for (B, nm), (nbytes,) in layout()["det"].items():                # [n 4 per item][current keypoints 8 per slot]
        assert nbytes == up256(4 * B) + 8 * nm * B


def test_point_block():
    for (B, nm), got in layout()["point"].items():
        s = nm * B
        o_n = 0; o_kps = up256(4 * B); o_pri = o_kps + 8 * s; o_flg = o_pri + 8 * s; in_bytes = up256(o_flg + s)
        o_out = in_bytes; o_st = o_out + 8 * s; o_unpx = up256(o_st + s); o_bv = up256(o_unpx + 8 * s); blk_bytes = o_bv + 24 * s
        assert got == (o_n, o_kps, o_pri, o_flg, in_bytes, o_out, o_st, o_unpx, o_bv, blk_bytes), (B, nm)
        # n, keypoints, priors, flags go up; positions, status, undistorted pixels, bearings come down
        _sections_ok([o_n, o_kps, o_pri, o_flg, o_out, o_st, o_unpx, o_bv], [4 * B, 8 * s, 8 * s, s, 8 * s, s, 8 * s, 24 * s], blk_bytes,
                     [True, True, False, False, True, False, True, True])
        assert in_bytes == o_out and in_bytes % 256 == 0
    assert layout()["point"][65535, 2048][-1] > 1 << 32               # (Python's integers do not wrap: a 32-bit product in the header would differ above)


def test_map_block():
    for (B, nm), got in layout()["map"].items():
        s = nm * B
        m_it = 0; m_T = up256(16 * B); m_w = up256(m_T + 56 * B); m_3d = up256(m_w + 24 * s); map_bytes = up256(m_3d + s)
        assert got == (m_it, m_T, m_w, m_3d, map_bytes), (B, nm)
        _sections_ok([m_it, m_T, m_w, m_3d], [16 * B, 56 * B, 24 * s, s], map_bytes, [True] * 4)
        assert map_bytes % 256 == 0
    assert layout()["map"][65535, 2048][-1] > 1 << 31


def test_pose_block():
    for (B, nm), got in layout()["pose"].items():
        s = nm * B
        q_T = 0; q_seed = up256(56 * B); q_fl = up256(q_seed + 8 * B); q_sc = up256(q_fl + B); q_in = up256(q_sc + 4 * s)
        q_out = q_in; q_ms = up256(q_out + POSE_OUT * B); q_rm = up256(q_ms + 8 * B); pose_bytes = up256(q_rm + s)
        assert got == (q_T, q_seed, q_fl, q_sc, q_in, q_out, q_ms, q_rm, pose_bytes), (B, nm)
        # pose, seed, flags, scale go up; the record, (m, rows), the removal bytes come down
        _sections_ok([q_T, q_seed, q_fl, q_sc, q_out, q_ms, q_rm], [56 * B, 8 * B, B, 4 * s, POSE_OUT * B, 8 * B, s], pose_bytes, [True] * 7)
        assert q_in == q_out and pose_bytes % 256 == 0


def test_epipolar_blocks():
    for (B, nm), got in layout()["epi"].items():
        s = nm * B
        e_lm = 0; e_nk = up256(4 * s); e_sd = up256(e_nk + 4 * B); e_in = up256(e_sd + 8 * B)
        e_out = e_in; e_nc = up256(e_out + EPIF_OUT * B); e_rm = up256(e_nc + 4 * B); e_er = up256(e_rm + s); e_pc = up256(e_er + 4 * s)
        epi_bytes = up256(e_pc + 4 * s)
        assert got == (e_lm, e_nk, e_sd, e_in, e_out, e_nc, e_rm, e_er, e_pc, epi_bytes), (B, nm)
        # lmid, nbkfs, seed go up; the record, n_cur, the removal bytes, the errors, the pairs come down
        _sections_ok([e_lm, e_nk, e_sd, e_out, e_nc, e_rm, e_er, e_pc], [4 * s, 4 * B, 8 * B, EPIF_OUT * B, 4 * B, s, 4 * s, 4 * s], epi_bytes,
                     [True] * 8)
        assert e_in == e_out and epi_bytes % 256 == 0
        x_slot = up256(KF_HDR * B); x_rank = x_slot + 4 * s; fx_bytes = x_rank + 4 * s
        assert layout()["fx"][B, nm] == (x_slot, x_rank, fx_bytes), (B, nm)
        _sections_ok([0, x_slot, x_rank], [KF_HDR * B, 4 * s, 4 * s], fx_bytes, [True, True, False])
