// framepose.hip -- the lock-step step's pose set on gfx950: what stands between k_compute_keypoints and computePose's chain
// (pose_dev.hpp) when the tracker runs both in one enqueue (ov2_btracker_track_frame_pose, trackb.hip).  The reference builds these
// arrays on the host (src/visual_front_end.cpp:675-712: the frame's 3-D keypoints after kltTracking removed the lost ones).
//   k_pose_select  one lane per slot: the byte the pack reads, (status & 3) == 1 && is3d.  A stage of its own, so that a later filter
//                  (epipolar2d2dFiltering) can clear bytes between the two without touching the pack.
//   k_pose_pack    ONE WAVEFRONT PER ITEM: stable compaction of the selected slots (ballot prefixes, slot order) out of the tracker's
//                  point block and map block into the chain's inputs at capacity (item b's points at b * n_max): unpx widened to
//                  double, the map point, sigma = 2^scale, the bearing; the slot of every packed point and the packed rank of every
//                  slot; PoseItem, P3Item; and, where the item searches, its sample table -- the integers of ov2_p3p_draw_samples:
//                  64 rows at a time, one per lane, each from the counter it starts at if no earlier row rejects a value; the rows up to
//                  the first rejection are right and are stored, the rest is drawn again from the corrected counter.
//   k_pose_unpack  one lane per slot, after k_pose_decide: the removal bytes from packed space to slot space through the ranks.
// Every count read from device memory is clamped against n_max before it indexes anything; a rank is checked before it is used.
#include "common.hpp"
#include "pose_dev.hpp"

#pragma clang fp contract(off)

#define FP_WALK 4096                    // values one row of the sample table may consume (see k_pose_pack)

struct FpArgs {
    // the tracker's blocks: n_max slots per item
    const int *n_dev; const uint8_t *status, *is3d; const float *unpx; const double *bv, *wpt;
    // the step's pose inputs: scale per slot; per item bit 0 p3p_req, bit 1 do_p3p; the seed
    const int *scale; const uint8_t *flags; const unsigned long long *seed;
    uint8_t *sel; int *slot, *rank; int2 *ms;           // per slot: selected, slot of packed point k, rank of slot i; per item {m, rows drawn}
    // the chain's inputs (PoseLayout)
    PoseItem *items; double *c_unpx, *c_sigma; P3Item *p3items; double *p3bv, *p3X; int4 *samples;
    const uint8_t *removed; uint8_t *removed_slot;      // packed space (the chain's) -> slot space
    int n_max, n_rows;
};

__device__ __forceinline__ int fp_count(const FpArgs &a, int b) { const int n = a.n_dev[b]; return n < 0 ? 0 : (n > a.n_max ? a.n_max : n); }

__global__ __launch_bounds__(256) void k_pose_select(FpArgs a)
{
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= fp_count(a, b)) return;
    const size_t s = (size_t)b * a.n_max + i;
    a.sel[s] = (uint8_t)((a.status[s] & 3) == 1 && a.is3d[s] != 0);
}

__device__ __forceinline__ unsigned long long fp_splitmix64(unsigned long long seed, unsigned long long j)      // p3p.hip: p3p_splitmix64
{
    unsigned long long z = seed + (j + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ __launch_bounds__(64) void k_pose_pack(FpArgs a)
{
    const int b = blockIdx.x, lane = threadIdx.x, nm = a.n_max;
    const int n = fp_count(a, b);
    const size_t o = (size_t)b * nm;                                // the item's first slot, and its first packed point (pt0)
    int m = 0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        const bool keep = i < n && a.sel[o + i];
        const unsigned long long mk = __ballot(keep);
        if (keep) {
            const int r = m + __popcll(mk & ((1ull << lane) - 1ull));
            const size_t d = o + (size_t)r, s = o + (size_t)i;
            a.c_unpx[2 * d] = (double)a.unpx[2 * s]; a.c_unpx[2 * d + 1] = (double)a.unpx[2 * s + 1];
            a.p3X[3 * d] = a.wpt[3 * s]; a.p3X[3 * d + 1] = a.wpt[3 * s + 1]; a.p3X[3 * d + 2] = a.wpt[3 * s + 2];
            a.p3bv[3 * d] = a.bv[3 * s]; a.p3bv[3 * d + 1] = a.bv[3 * s + 1]; a.p3bv[3 * d + 2] = a.bv[3 * s + 2];
            a.c_sigma[d] = ldexp(1.0, a.scale[s]);
            a.slot[d] = i;
            a.rank[s] = r;
        } else if (i < n) a.rank[o + i] = -1;
        m += __popcll(mk);
    }
    const int fl = a.flags[b];
    const bool search = (fl & 2) && m >= 4;
    int rows = 0;
    if (search && a.n_rows > 0) {
        // ov2_p3p_draw_samples(seed, m, n_rows): v_j = splitmix64(seed, j) % m in order of j, a value already in the row is skipped.
        // m <= 2048: z % m from 32-bit pieces, ((hi % m) * (2^32 % m) + lo % m) % m, every term below 2^23.
        const unsigned um = (unsigned)m, two32 = (0xffffffffu % um + 1u) % um;
        const unsigned long long seed = a.seed[b];
        int4 *tab = a.samples + (size_t)b * a.n_rows;
        // Sixty-four rows at a time, on the assumption that none of them rejects a value: lane l draws row (rows + l) from counter
        // j0 + 4 l and walks on until it holds four distinct values.  The assumption is right for the lanes up to AND INCLUDING the
        // first that consumed more than four values; they are stored, j0 moves past what they consumed, the others are drawn again.
        // (A rejection costs a pass: about m / 6 rows per pass for m >> 4, one row per pass at m = 4.  A walk on one lane over
        // every value took 166 us for 200 rows of m = 215; this takes a few passes.)  Bounds: FP_WALK values per row -- a row of
        // m >= 4 that needs more has probability (3/4)^4000 -- and n_rows + 8 passes; they only keep the loops finite.
        unsigned long long j0 = 0;
        for (int pass = 0; rows < a.n_rows && pass < a.n_rows + 8; pass++) {
            const unsigned long long j = j0 + 4ull * (unsigned long long)lane;
            int c0 = 0, c1 = 0, c2 = 0, c3 = 0, k = 0, cnt = 0;
            while (k < 4 && cnt < FP_WALK) {
                const unsigned long long z = fp_splitmix64(seed, j + (unsigned long long)cnt);
                const unsigned hi = (unsigned)(z >> 32), lo = (unsigned)z;
                const int x = (int)(((hi % um) * two32 + lo % um) % um);
                cnt++;
                const bool dup = (k > 0 && x == c0) || (k > 1 && x == c1) || (k > 2 && x == c2);
                if (!dup) { if (k == 0) c0 = x; else if (k == 1) c1 = x; else if (k == 2) c2 = x; else c3 = x; k++; }
            }
            const unsigned long long moved = __ballot(cnt != 4);
            const int first = moved ? __ffsll((long long)moved) - 1 : 64;
            const int k_first = __shfl(k, first & 63), cnt_first = __shfl(cnt, first & 63);
            int take = first < 64 ? first + (k_first == 4 ? 1 : 0) : 64;
            take = take < a.n_rows - rows ? take : a.n_rows - rows;
            if (take <= 0) break;                                    // (a row beyond FP_WALK: the table ends here)
            if (lane < take) tab[rows + lane] = make_int4(c0, c1, c2, c3);
            j0 += take == first + 1 ? 4ull * (unsigned long long)first + (unsigned long long)cnt_first : 4ull * (unsigned long long)take;
            rows += take;
        }
    }
    if (lane == 0) {
        a.items[b] = PoseItem{m, (int)o, (fl & 2) != 0, fl & 1};
        a.p3items[b] = P3Item{search ? m : 0, rows, (int)o, (int)((size_t)b * a.n_rows)};
        a.ms[b] = make_int2(m, rows);
    }
}

__global__ __launch_bounds__(256) void k_pose_unpack(FpArgs a)
{
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= fp_count(a, b)) return;
    const size_t o = (size_t)b * a.n_max;
    const int r = a.rank[o + i];
    a.removed_slot[o + i] = (r >= 0 && r < a.n_max) ? a.removed[o + (size_t)r] : (uint8_t)0;
}

// The pose half of a lock-step step behind k_compute_keypoints on `s` (pose_dev.hpp: FramePoseIo).  Without a hook the launches are
// the four below.
int ov2_launch_frame_pose(hipStream_t s, const ov2_pose_params *params, const PoseLayout &L, int n_active, bool search, const FramePoseIo &io,
                          ov2_fp_hook hook, void *hook_arg)
{
    const size_t NP = L.pl.NP;
    uint8_t *work = io.work, *x = work + L.total;
    FpArgs a;
    a.n_dev = io.n_dev; a.status = io.status; a.is3d = io.is3d; a.unpx = io.unpx; a.bv = io.bv; a.wpt = io.wpt;
    a.scale = io.scale; a.flags = io.flags; a.seed = io.seed;
    a.sel = x; a.slot = (int *)(x + ((NP + 15) & ~(size_t)15)); a.rank = a.slot + NP; a.ms = (int2 *)io.ms;
    uint8_t *p3 = work + L.o_p3;
    a.items = (PoseItem *)(work + L.o_it); a.c_unpx = (double *)(work + L.o_px); a.c_sigma = (double *)(work + L.o_sg);
    a.p3items = (P3Item *)(p3 + L.pl.o_it); a.p3bv = (double *)(p3 + L.pl.o_bv); a.p3X = (double *)(p3 + L.pl.o_X); a.samples = (int4 *)(p3 + L.pl.o_sm);
    a.removed = work + L.o_rm; a.removed_slot = io.removed_slot;
    a.n_max = L.n_max; a.n_rows = L.n_rows;
    const dim3 slots((L.n_max + 255) / 256, n_active);
    hipLaunchKernelGGL(k_pose_select, slots, dim3(256), 0, s, a);
    OV2_HIP_CHECK(hipGetLastError());
    if (hook) { const int rch = hook(s, a.sel, hook_arg);  if (rch != OV2_OK) return rch; }
    hipLaunchKernelGGL(k_pose_pack, dim3(n_active), dim3(64), 0, s, a);
    OV2_HIP_CHECK(hipGetLastError());
    const int rc = pose_chain_enqueue(s, params, L, work, io.Twc, io.out, n_active, search);
    if (rc != OV2_OK) return rc;
    hipLaunchKernelGGL(k_pose_unpack, slots, dim3(256), 0, s, a);
    OV2_HIP_CHECK(hipGetLastError());
    return OV2_OK;
}

size_t ov2_frame_pose_work_bytes(const PoseLayout &L) { return L.total + ((L.pl.NP + 15) & ~(size_t)15) + 8 * L.pl.NP + 16; }
size_t ov2_frame_pose_slot_offset(const PoseLayout &L) { return L.total + ((L.pl.NP + 15) & ~(size_t)15); }
