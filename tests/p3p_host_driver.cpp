// Host build of csrc/p3p.hpp (the code k_p3p and k_pose_estimate run):
//   p3p_host_driver IN OUT
// IN: n triplets, 18 doubles each (9 bearings, 9 world points).  OUT per
// triplet 49 doubles: the count, then four poses (NaN beyond the count).
#include <cstdio>
#include <vector>

#include "p3p.hpp"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 3;
    std::vector<double> buf;
    double rec[18];
    while (std::fread(rec, sizeof(double), 18, in) == 18) buf.insert(buf.end(), rec, rec + 18);
    std::fclose(in);
    const size_t n = buf.size() / 18;
    std::vector<double> out(49 * n);
    for (size_t i = 0; i < n; ++i)
        out[49 * i] = acm::p3p::solve(&buf[18 * i], &buf[18 * i + 9], &out[49 * i + 1]);
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 4;
    const bool ok = std::fwrite(out.data(), sizeof(double), out.size(), o) == out.size();
    std::fclose(o);
    return ok ? 0 : 5;
}
