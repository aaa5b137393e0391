// motion_run.cpp -- test driver for the motion model through the C++ adapter (ov2slam_amd/host/visual_front_end.hpp): reads the case
// file written by tests/test_gpu_motion.py (per frame the pose handed to applyMotionModel, the pose handed to updateMotionModel and
// the time), plays the frames through one ov2::MotionModel and writes per frame the predicted pose, its inverse, resynced and the
// model's state after the update.  File format (both ways): a sequence of arrays, each an int64 byte count followed by the raw bytes.
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include "../../ov2slam_amd/host/visual_front_end.hpp"

template <class T> static std::vector<T> rd(FILE *f)
{
    long long nb = 0;
    if (fread(&nb, 8, 1, f) != 1) throw std::runtime_error("short case file");
    std::vector<T> v((size_t)nb / sizeof(T));
    if (nb && fread(v.data(), 1, (size_t)nb, f) != (size_t)nb) throw std::runtime_error("short case file");
    return v;
}
template <class T> static void wr(FILE *f, const T *p, size_t n)
{
    const long long nb = (long long)(n * sizeof(T));
    fwrite(&nb, 8, 1, f);
    if (nb) fwrite(p, 1, (size_t)nb, f);
}

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: motion_run <case> <result>\n"); return 2; }
    try {
        FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
        if (!fi || !fo) throw std::runtime_error("cannot open files");
        const std::vector<double> A = rd<double>(fi), U = rd<double>(fi), times = rd<double>(fi);
        const size_t n = times.size();
        if (A.size() != 7 * n || U.size() != 7 * n) throw std::runtime_error("case arrays differ in length");
        ov2::Context ctx(0);
        ov2::MotionModel mm;
        std::vector<double> pred(7 * n), inv(7 * n), states(14 * n);
        std::vector<uint8_t> resynced(n);
        for (size_t k = 0; k < n; k++) {
            double T[7];
            for (int j = 0; j < 7; j++) T[j] = A[7 * k + j];
            bool rs = false;
            if (mm.applyMotionModel(ctx, T, times[k], &inv[7 * k], &rs) != OV2_OK) throw std::runtime_error(std::string("applyMotionModel: ") + ov2_last_error());
            for (int j = 0; j < 7; j++) pred[7 * k + j] = T[j];
            resynced[k] = rs ? 1 : 0;
            if (mm.updateMotionModel(ctx, &U[7 * k], times[k]) != OV2_OK) throw std::runtime_error(std::string("updateMotionModel: ") + ov2_last_error());
            const ov2_motion_state &s = mm.state();
            states[14 * k] = s.prev_time;
            for (int j = 0; j < 7; j++) states[14 * k + 1 + j] = s.prevTwc[j];
            for (int j = 0; j < 6; j++) states[14 * k + 8 + j] = s.log_relT[j];
        }
        // a refused call leaves the model where it was
        double T[7] = {0, 0, 0, 0, 0, 0, 1};
        const ov2_motion_state before = mm.state();
        const int refused = (mm.applyMotionModel(ctx, T, times[n - 1]) == OV2_EINVAL && mm.updateMotionModel(ctx, T, times[n - 1] - 1.) == OV2_EINVAL &&
                             memcmp(&before, &mm.state(), sizeof before) == 0) ? 1 : 0;
        wr(fo, pred.data(), pred.size()); wr(fo, inv.data(), inv.size()); wr(fo, resynced.data(), resynced.size());
        wr(fo, states.data(), states.size()); wr(fo, &refused, 1);
        fclose(fi); fclose(fo);
    } catch (const std::exception &ex) {
        fprintf(stderr, "%s\n", ex.what());
        return 1;
    }
    return 0;
}
