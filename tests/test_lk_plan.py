"""The unit plan of the persistent k_fb_klt3 (ov2slam_amd/csrc/lk_plan.hpp): the 8 lists together must hold every
(item, block) with block * 20 < n[item] exactly once and nothing else (a hole leaves keypoints untracked, a double entry
tracks them twice into the same slots), each list in ascending item order, every unit on the list of the residue that
ov2_xcd_map gives its work-group id, and no list longer than the room the launcher reserves for it.  The header is plain C++;
it is compiled here with g++ like tests/test_xcd_map.py does for its header.

Cases: batch 1..20, nbx 1..4, counts from {0, 1, 19, 20, 21, n_max}.  The full product has 6^batch vectors per size; it is
walked completely up to batch 8 (1.7 M vectors: a whole group of 8 items, and every left-over count 1..7 on its own).  An
entry of a list depends on the count of its own item only (ov2_lkp_entry_of), so beyond that the vectors are: all items at one
value, one item at each other value in each position (6 x 6 x batch), and 2000 seeded random draws per (batch, nbx)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <cstdio>
#include <vector>
#include "xcd_map.hpp"
#include "lk_plan.hpp"
static const int KPB = 20;
static int check(int batch, int nbx, const int *n, int n_all)
{
    // work-group id of every (item, block) under the direct form's map
    static std::vector<int> id_of;
    static int id_batch = -1, id_nbx = -1;
    if (id_batch != batch || id_nbx != nbx) {
        id_of.assign((size_t)batch * nbx, -1);
        for (int id = 0; id < batch * nbx; id++) { int it, k; ov2_xcd_map(id, nbx, batch, &it, &k); id_of[(size_t)it * nbx + k] = id; }
        id_batch = batch; id_nbx = nbx;
    }
    const int cap = ov2_lkp_list_cap(batch, nbx);
    std::vector<int> seen((size_t)batch * nbx, 0), list((size_t)cap + 64, -7);
    for (int r = 0; r < OV2_LKP_LISTS; r++) {
        const int len = ov2_lkp_fill_list(r, n, n_all, batch, nbx, KPB, list.data());
        if (len < 0 || len > cap) return 1;
        int prev_item = -1, prev_id = -1;
        for (int u = 0; u < len; u++) {
            int item, block;
            ov2_lkp_unpack(list[u], nbx, &item, &block);
            if (item < 0 || item >= batch || block < 0 || block >= nbx) return 2;
            if (!(block * KPB < (n ? n[item] : n_all))) return 3;                 // nothing but real units
            if (seen[(size_t)item * nbx + block]++) return 4;                      // exactly once
            if (item < prev_item) return 5;                                        // ascending item order
            const int id = id_of[(size_t)item * nbx + block];
            if ((id & 7) != r) return 6;                                           // where ov2_xcd_map puts it
            if (id <= prev_id) return 7;                                           // in the order of the ids: blocks of an item consecutive
            prev_item = item; prev_id = id;
        }
    }
    for (int item = 0; item < batch; item++)
        for (int block = 0; block < nbx; block++)
            if (block * KPB < (n ? n[item] : n_all) && !seen[(size_t)item * nbx + block]) return 8;   // every unit
    return 0;
}
int main()
{
    unsigned long long rng = 88172645463325252ull;
    for (int nbx = 1; nbx <= 4; nbx++) {
        const int n_max = KPB * nbx - 3;
        const int vals[6] = {0, 1, 19, 20, 21, n_max};
        for (int batch = 1; batch <= 20; batch++) {
            std::vector<int> n(batch, 0);
            auto run = [&]() {
                if (int rc = check(batch, nbx, n.data(), n_max)) {
                    printf("FAIL batch %d nbx %d rc=%d n =", batch, nbx, rc);
                    for (int v : n) printf(" %d", v);
                    printf("\n");
                    return 1;
                }
                return 0;
            };
            if (check(batch, nbx, nullptr, n_max)) { printf("FAIL batch %d nbx %d n == NULL\n", batch, nbx); return 1; }
            if (batch <= 8) {
                long long total = 1;
                for (int i = 0; i < batch; i++) total *= 6;
                for (long long c = 0; c < total; c++) {
                    long long t = c;
                    for (int i = 0; i < batch; i++) { n[i] = vals[t % 6]; t /= 6; }
                    if (run()) return 1;
                }
            } else {
                for (int a = 0; a < 6; a++)
                    for (int b = 0; b < 6; b++)
                        for (int pos = 0; pos < batch; pos++) {
                            for (int i = 0; i < batch; i++) n[i] = vals[a];
                            n[pos] = vals[b];
                            if (run()) return 1;
                        }
                for (int k = 0; k < 2000; k++) {
                    for (int i = 0; i < batch; i++) { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; n[i] = vals[rng % 6]; }
                    if (run()) return 1;
                }
            }
        }
    }
    // the bench geometries: 4096 items, stride 308 (16 blocks), 216 and 92 keypoints each; a ragged one
    {
        std::vector<int> n(4096);
        for (int v : {216, 92}) { for (auto &x : n) x = v; if (check(4096, 16, n.data(), 308)) { printf("FAIL bench %d\n", v); return 1; } }
        for (int i = 0; i < 4091; i++) n[i] = (i * 37) % 309;
        if (check(4091, 16, n.data(), 308)) { printf("FAIL ragged\n"); return 1; }
    }
    printf("OK\n");
    return 0;
}
"""


def test_lk_plan_lists_every_unit_once(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text(SRC)
    exe = tmp_path / "t"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "ov2slam_amd", "csrc"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "OK", out.stdout + out.stderr
