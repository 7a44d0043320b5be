// Host build of csrc/essential.hpp (the code k_relative_pose_8pt and
// k_relative_pose run):
//   essential_host_driver IN OUT ROWS
// IN: problems of ROWS matches, 6 ROWS doubles each (the 3 ROWS bearings of
// image A, then those of image B).  OUT per problem 22 doubles: the number of
// matches in front, the pose (12), the essential matrix (9).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "essential.hpp"

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
    std::vector<double> out(22 * n);
    for (size_t i = 0; i < n; ++i) {
        const double* a = &buf[6 * rows * i];
        out[22 * i] = acm::essential::solve(rows, a, a + 3 * rows, &out[22 * i + 1], &out[22 * i + 13]);
    }
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 4;
    const bool ok = std::fwrite(out.data(), sizeof(double), out.size(), o) == out.size();
    std::fclose(o);
    return ok ? 0 : 5;
}
