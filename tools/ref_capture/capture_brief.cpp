// capture_brief.cpp -- OpenCV contrib's BriefDescriptorExtractor (the detector describeBRIEF creates at
// /root/reference/src/feature_extractor.cpp:243: 32 bytes, no orientation) on the input sets tools/brief_probe.py writes; dumps, per
// set, <name>.desc.npy (n_images x k x 32 uint8: row i of image j = keypoint i's descriptor, zero where OpenCV dropped the point) and
// <name>.valid.npy (n_images x k uint8).  Nothing else: the recovery of the test pairs and the comparison are
// tools/brief_pattern_from_probes.py and tests/test_brief_reference.py.  Needs OpenCV with the contrib modules (see CMakeLists.txt).
#include <opencv2/core.hpp>
#include <opencv2/xfeatures2d.hpp>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

static void save_npy(const std::string &path, const std::vector<uint8_t> &data, const std::vector<size_t> &shape)
{
    std::string dims;
    for (size_t d : shape) dims += std::to_string(d) + ",";
    std::string hdr = "{'descr': '|u1', 'fortran_order': False, 'shape': (" + dims + "), }";
    while ((10 + hdr.size() + 1) % 64) hdr += ' ';
    hdr += '\n';
    std::ofstream f(path, std::ios::binary);
    const uint16_t len = (uint16_t)hdr.size();
    f.write("\x93NUMPY\x01\x00", 8);
    f.write((const char *)&len, 2);
    f.write(hdr.data(), (std::streamsize)hdr.size());
    f.write((const char *)data.data(), (std::streamsize)data.size());
    if (!f) throw std::runtime_error("cannot write " + path);
}

template <class T> static std::vector<T> read_all(const std::string &path, size_t count)
{
    std::vector<T> v(count);
    std::ifstream f(path, std::ios::binary);
    f.read((char *)v.data(), (std::streamsize)(count * sizeof(T)));
    if (!f) throw std::runtime_error("short or missing " + path);
    return v;
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: ov2_capture_brief <input dir (tools/brief_probe.py)> <output dir>\n"); return 2; }
    const std::string in = argv[1], out = argv[2];
    try {
        cv::Ptr<cv::DescriptorExtractor> brief = cv::xfeatures2d::BriefDescriptorExtractor::create();
        std::ifstream man(in + "/sets.txt");
        if (!man) throw std::runtime_error("no sets.txt in " + in);
        std::string line;
        while (std::getline(man, line)) {
            std::istringstream ss(line);
            std::string name; size_t n = 0, w = 0, h = 0, k = 0;
            if (!(ss >> name >> n >> w >> h >> k)) continue;
            const std::vector<uint8_t> imgs = read_all<uint8_t>(in + "/" + name + ".img", n * w * h);
            const std::vector<float> kp = read_all<float>(in + "/" + name + ".kp", 2 * k);
            std::vector<uint8_t> desc(n * k * 32, 0), valid(n * k, 0);
            for (size_t j = 0; j < n; j++) {
                cv::Mat im((int)h, (int)w, CV_8UC1, (void *)(imgs.data() + j * w * h));
                std::vector<cv::KeyPoint> kps;
                for (size_t i = 0; i < k; i++) {
                    cv::KeyPoint p(cv::Point2f(kp[2 * i], kp[2 * i + 1]), 1.f);      // cv::KeyPoint::convert's defaults
                    p.class_id = (int)i;                                              // which point survived runByImageBorder
                    kps.push_back(p);
                }
                cv::Mat d;
                brief->compute(im, kps, d);
                for (size_t r = 0; r < kps.size(); r++) {
                    const size_t i = (size_t)kps[r].class_id;
                    valid[j * k + i] = 1;
                    for (int b = 0; b < 32; b++) desc[(j * k + i) * 32 + b] = d.at<uint8_t>((int)r, b);
                }
            }
            save_npy(out + "/" + name + ".desc.npy", desc, {n, k, 32});
            save_npy(out + "/" + name + ".valid.npy", valid, {n, k});
            printf("%s: %zu images x %zu keypoints\n", name.c_str(), n, k);
        }
    } catch (const std::exception &e) {
        fprintf(stderr, "ov2_capture_brief: %s\n", e.what());
        return 1;
    }
    return 0;
}
