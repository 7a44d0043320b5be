// Host build of csrc/homography.hpp (the code k_homography_4pt and
// k_homography run):
//   homography_host_driver IN OUT ROWS
// IN: problems of ROWS matches, 6 ROWS doubles each (the 3 ROWS bearings of
// image A, then those of image B).  OUT per problem 45 doubles: the number of
// solutions, H (9), the two poses (24), the two planes (8), tau, n_front (2).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "homography.hpp"

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    const long long rows = std::atoll(argv[3]);
    if (rows < 1) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 3;
    std::vector<double> buf, rec(6 * rows);
    while (std::fread(rec.data(), sizeof(double), rec.size(), in) == rec.size())
        buf.insert(buf.end(), rec.begin(), rec.end());
    std::fclose(in);
    const size_t n = buf.size() / rec.size();
    std::vector<double> out(45 * n);
    for (size_t i = 0; i < n; ++i) {
        const double* a = &buf[6 * rows * i];
        double* o = &out[45 * i];
        unsigned front[2];
        o[0] = acm::homography::solve(rows, a, a + 3 * rows, o + 1, o + 10, o + 34, o + 42, front);
        o[43] = front[0];
        o[44] = front[1];
    }
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 4;
    const bool ok = std::fwrite(out.data(), sizeof(double), out.size(), o) == out.size();
    std::fclose(o);
    return ok ? 0 : 5;
}
