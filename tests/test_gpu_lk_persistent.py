"""The persistent form of k_fb_klt3 (lk3.hip, OV2_OPT_LK_PERSIST): a plan kernel lists the (item, keypoint block) units that
hold a keypoint and a fixed number of work-groups pull them.  Results must be bit for bit those of the direct form and of the
oracle for every number of work-groups, slots beyond n_per_item stay untouched, and plan and counters are re-made by every call.

19 image pairs (more than 8, no multiple of 8: whole groups and left-over items of the XCD map) of 264 x 100, 45 keypoint
slots per item (3 blocks of 20), ragged counts.  With 1 and 5 work-groups there are fewer work-groups than units, so the pull
loop and the taking from other lists run; 1 runs every unit in one wavefront.  One case runs the default rule (-1) on a stride
with more keypoint blocks than a device holds work-groups at once, the path that ships as the default.  All cases run in ONE child process (torch owns the
device buffers and has to initialise HIP first) that reports per case; the oracle's results are computed once and shared."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

PERSIST = (0, 1, 5, 64)
LEVELS = (3, 1)
CASES = (["persist%d_lvl%d" % (p, l) for p in PERSIST for l in LEVELS] + ["same_for_every_grid", "all_counts_zero", "n_per_item_null",
         "two_calls_back_to_back", "auto_rule_large_stride"])

_SCRIPT = r"""
import ctypes as C, json, sys, numpy as np
import torch
torch.cuda.init()
sys.path.insert(0, sys.argv[1])
import ov2slam_amd
from ov2slam_amd import synth, _lib as L
from oracle import oracle as O
PERSIST, LEVELS = (0, 1, 5, 64), (3, 1)
ctx = ov2slam_amd.Context(0)
ctx.set_option(L.OV2_OPT_LK_IMPL, L.OV2_LK_IMPL_LANE3)
B, NMAX, W, H = 19, 45, 264, 100
rng = np.random.default_rng(17)
N_A = np.array([45, 0, 1, 19, 20, 21, 40, 41, 45, 7, 33, 45, 0, 20, 41, 1, 45, 21, 19], np.int32)
N_B = np.array([0, 45, 21, 1, 41, 20, 19, 40, 0, 45, 2, 0, 45, 39, 1, 20, 22, 45, 40], np.int32)
prevs, curs, kps, pri = [], [], np.zeros((B, NMAX, 2), np.float32), np.zeros((B, NMAX, 2), np.float32)
for b in range(B):
    p, c, flow = synth.frame_pair(W, H, seed=70 + b, shift=(1.2 + b * 0.2, -0.8), theta=0.0015 * b)
    prevs.append(p); curs.append(c)
    g = synth.grid_keypoints(W, H, 15, rng)
    k = g[rng.permutation(len(g))][:NMAX]
    assert len(k) == NMAX
    kps[b] = k; pri[b] = (flow(k) + rng.normal(0, 1.0, k.shape)).astype(np.float32)
Pp = ov2slam_amd.Pyramid(ctx, W, H, 9, 3, batch=B).build(np.stack(prevs))
Pc = ov2slam_amd.Pyramid(ctx, W, H, 9, 3, batch=B).build(np.stack(curs))
ctx.sync()
Rp = [O.Pyramid(x, 9, 3) for x in prevs]; Rc = [O.Pyramid(x, 9, 3) for x in curs]
vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
_ref = {}
def ref(lvl, b, n):                       # the oracle on the first n keypoints of item b: (positions, status, iterations)
    if (lvl, b, n) not in _ref:
        rp, rs, rstats = O.fb_klt(Rp[b], Rc[b], 9, lvl, 30.0, 0.5, kps[b, :n], pri[b, :n]) if n else (np.zeros((0, 2), np.float32), np.zeros(0, bool), (0, 0))
        _ref[(lvl, b, n)] = (rp, rs, int(rstats[0]))
    return _ref[(lvl, b, n)]
dk = torch.from_numpy(kps).cuda()
class Call:
    # one ov2_fb_klt_d with its own in/out buffers; nothing synchronises here
    def __init__(self, lvl, counts):
        self.lvl, self.counts = lvl, counts
        self.dk = dk
        self.dp = torch.from_numpy(pri).cuda()
        self.dn = torch.from_numpy(counts).cuda() if counts is not None else None
        self.st = torch.full((B, NMAX), 7, dtype=torch.uint8, device="cuda")
        self.stats = torch.zeros(2, dtype=torch.int64, device="cuda")
    def launch(self):
        L.check(ctx.lib.ov2_fb_klt_d(ctx.h, Pp.h_pyr, Pc.h_pyr, 9, self.lvl, 30, 0.01, 30.0, 0.5, vp(self.dk), vp(self.dp), self.st.shape[1], vp(self.dn), vp(self.st), vp(self.stats)))
        return self
    def check(self):
        gp, gs = self.dp.cpu().numpy(), self.st.cpu().numpy()
        tot = 0
        for b in range(B):
            n = NMAX if self.counts is None else int(self.counts[b])
            rp, rs, it = ref(self.lvl, b, n)
            assert np.array_equal(gs[b, :n].astype(bool), rs) and np.all(gs[b, :n] <= 1), ("status", b)
            assert np.array_equal(gp[b, :n].view(np.uint32), rp.view(np.uint32)), ("positions", b)
            assert np.all(gs[b, n:] == 7) and np.array_equal(gp[b, n:].view(np.uint32), pri[b, n:].view(np.uint32)), ("slots beyond n_per_item", b)
            tot += it
        assert int(self.stats[0].item()) == tot, ("iterations", int(self.stats[0].item()), tot)
        return gp, gs
def sync():
    torch.cuda.synchronize(); ctx.sync()
results, outs = {}, {}
def case(name, fn):
    try:
        fn(); results[name] = "ok"
    except (AssertionError, KeyError) as e:      # a wrong result of one case does not hide the others; a HIP error ends the run
        results[name] = "%s: %s" % (type(e).__name__, e)
    print("CASE " + json.dumps([name, results[name]]), flush=True)
sync()
for persist in PERSIST:
    for lvl in LEVELS:
        def run(persist=persist, lvl=lvl):
            ctx.set_option(L.OV2_OPT_LK_PERSIST, persist)
            c = Call(lvl, N_A); sync(); c.launch(); sync()
            outs[(persist, lvl)] = c.check()
        case("persist%d_lvl%d" % (persist, lvl), run)
def same():
    for lvl in LEVELS:
        for persist in PERSIST[1:]:
            for a, b in zip(outs[(PERSIST[0], lvl)], outs[(persist, lvl)]):
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (persist, lvl)
case("same_for_every_grid", same)
def zeros():
    for persist in PERSIST:
        ctx.set_option(L.OV2_OPT_LK_PERSIST, persist)
        c = Call(3, np.zeros(B, np.int32)); sync(); c.launch(); sync()
        assert np.all(c.st.cpu().numpy() == 7) and np.array_equal(c.dp.cpu().numpy().view(np.uint32), pri.view(np.uint32)), persist
        assert c.stats.tolist() == [0, 0], persist
case("all_counts_zero", zeros)
def null_counts():
    for persist in PERSIST:
        ctx.set_option(L.OV2_OPT_LK_PERSIST, persist)
        c = Call(3, None); sync(); c.launch(); sync(); c.check()
case("n_per_item_null", null_counts)
def back_to_back():
    for persist in (5, 64):
        ctx.set_option(L.OV2_OPT_LK_PERSIST, persist)
        c1, c2 = Call(3, N_A), Call(1, N_B); sync()
        c1.launch(); c2.launch(); sync()
        c1.check(); c2.check()
case("two_calls_back_to_back", back_to_back)
def auto_rule():
    # The default rule on its persistent side: more keypoint blocks (19 x 820 = 15 580) than a device holds work-groups at once
    # (256 CUs x 16 = 4096 on MI355X; no device of this family holds 15 580), so the occupancy query runs and one round of resident
    # work-groups pulls the 34 real units.  Same keypoints in the first 45 slots of a 16 400-slot stride, same oracle results.
    BIG = 16400
    ctx.set_option(L.OV2_OPT_LK_PERSIST, -1)
    c = Call(3, N_A)
    kb = np.zeros((B, BIG, 2), np.float32); kb[:, :NMAX] = kps
    pb = np.full((B, BIG, 2), -5.0, np.float32); pb[:, :NMAX] = pri
    c.dk = torch.from_numpy(kb).cuda(); c.dp = torch.from_numpy(pb).cuda()
    c.st = torch.full((B, BIG), 7, dtype=torch.uint8, device="cuda")
    sync(); c.launch(); sync()
    gp, gs = c.dp.cpu().numpy(), c.st.cpu().numpy()
    assert np.all(gs[:, NMAX:] == 7) and np.array_equal(gp[:, NMAX:].view(np.uint32), pb[:, NMAX:].view(np.uint32)), "slots beyond the 45th"
    c.dp, c.st = torch.from_numpy(np.ascontiguousarray(gp[:, :NMAX])), torch.from_numpy(np.ascontiguousarray(gs[:, :NMAX]))
    for a, b in zip(c.check(), outs[(0, 3)]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
case("auto_rule_large_stride", auto_rule)
print("DONE")
"""


@pytest.fixture(scope="module")
def child_results():
    pytest.importorskip("torch")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _SCRIPT, root], capture_output=True, text=True, timeout=600)
    res = dict(json.loads(line[5:]) for line in r.stdout.splitlines() if line.startswith("CASE "))
    return res, r.returncode, r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.parametrize("name", CASES)
def test_lk_persistent(child_results, name):
    res, rc, tail = child_results
    assert name in res, "the child process ended before this case (exit %d)\n%s" % (rc, tail)
    assert res[name] == "ok", res[name]
