"""bench.py's seeded inputs on CPU: make_inputs() (the arithmetic on the random draws done for all sequences of a transition at
once) returns, bit for bit, what the straightforward per-texture / per-sequence loop below returns for
the same seed."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def loop_inputs(b, seqs, seed):
    """The reference: one texture, one sequence at a time, on bench module b's sizes.  Returns (views, kps, pri, pri_uniform)."""
    from ov2slam_amd import synth
    W, H, NF, NKPS = b.W, b.H, b.NF, b.NKPS
    rng = np.random.default_rng(seed)
    n_sets = max(1, min(b.N_VIEW_SETS, seqs))
    n_tex = (n_sets + 3) // 4
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    views = np.zeros((n_sets, NF + 1, H, W), np.uint8)
    offs_of = []
    for t in range(n_tex):
        tex = synth.base_texture(1400, seed + 101 * t, nblobs=int(rng.integers(200, 900)))
        offs = []
        ox, oy, th = float(rng.uniform(100, 250)), float(rng.uniform(100, 250)), float(rng.uniform(-0.05, 0.05))
        base = []
        for _ in range(NF + 1):
            base.append(synth.warp(tex, W, H, ox, oy, th)); offs.append((ox, oy, th))
            ox += rng.uniform(-5, 5); oy += rng.uniform(-4, 4); th += rng.uniform(-0.006, 0.006)
        base = np.stack(base).astype(np.float32)
        for v in range(4):
            k = 4 * t + v
            if k >= n_sets:
                break
            img = (base, base * 0.35 + 90.0, 255.0 * (base / 255.0) ** 2.2, 255.0 - base * 0.8)[v]
            views[k] = np.clip(np.rint(img), 0, 255).astype(np.uint8)
            offs_of.append(offs)
    if n_sets >= 8:
        k = n_sets - 1
        sel = rng.uniform(size=views[k].shape) < 0.8
        views[k] = np.where(sel, views[k] // 32, views[k] // 4).astype(np.uint8)

    def flow(offs, pts, a, b_):
        (ox0, oy0, t0), (ox1, oy1, t1) = offs[a], offs[b_]
        dx, dy = pts[:, 0] - cx, pts[:, 1] - cy
        c, s = np.cos(t0), np.sin(t0)
        tx, ty = c * dx - s * dy + cx + ox0, s * dx + c * dy + cy + oy0
        dx, dy = tx - cx - ox1, ty - cy - oy1
        c, s = np.cos(-t1), np.sin(-t1)
        return np.stack([c * dx - s * dy + cx, s * dx + c * dy + cy], 1)

    kps = np.zeros((2 * NF, seqs, NKPS, 2), np.float32)
    pri = np.zeros_like(kps)
    pri_u = np.zeros_like(kps)
    for f in range(2 * NF):
        va, vb = b.walk_view(f), b.walk_view(f + 1)
        for s in range(seqs):
            k = synth.grid_keypoints(W, H, b.CELL, rng)[:NKPS]
            if len(k) < NKPS:
                extra = np.stack([rng.uniform(20, W - 20, NKPS - len(k)), rng.uniform(20, H - 20, NKPS - len(k))], 1)
                k = np.concatenate([k, extra.astype(np.float32)])
            rng.shuffle(k)
            kps[f, s] = k
            noise = rng.normal(0, 1.5, k.shape)
            pri[f, s] = flow(offs_of[s % n_sets], k.astype(np.float64), va, vb) + noise
            pri_u[f, s] = flow(offs_of[0], k.astype(np.float64), va, vb) + noise
    return views, kps, pri, pri_u


@pytest.mark.parametrize("workload, seqs, seed", [("euroc", 9, 77), ("kitti", 5, 5)])
def test_make_inputs_matches_the_per_sequence_loop(workload, seqs, seed):
    b = _bench()
    if workload == "kitti":                                   # the sizes main() sets for --workload kitti
        b.W, b.H, b.NKPS = 1241, 376, 396
    want = loop_inputs(b, seqs, seed)
    got = b.make_inputs(seqs, seed, uniform=True)
    assert len(got) == 4
    for name, g, w in zip(("views", "kps", "pri", "pri_uniform"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), name
    plain = b.make_inputs(seqs, seed)
    assert len(plain) == 3 and all(np.array_equal(g, w) for g, w in zip(plain, want))
