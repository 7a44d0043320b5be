// Host build of csrc/similarity.hpp (the code k_similarity_3pt and
// k_similarity run):
//   similarity_host_driver IN OUT ROWS RIGID MODE
// IN: problems of ROWS correspondences, 6 ROWS doubles each (the ROWS points
// a, then the ROWS points b).  OUT per problem 14 doubles: the count 0 or 1,
// then the similarity (R row-major, t, s).  MODE 3pt: similarity_3pt (ROWS =
// 3).  MODE fit: the refit's arithmetic -- one pass for the centroids, one for
// the centred sums, in index order, then fit.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "similarity.hpp"

namespace sim = acm::similarity;

static bool fit_rows(long long rows, const double* a, const double* b, bool rigid,
                     double (&S)[sim::kDoubles]) {
    double am[3] = {0.0, 0.0, 0.0}, bm[3] = {0.0, 0.0, 0.0};
    for (long long j = 0; j < rows; ++j)
        for (int k = 0; k < 3; ++k) {
            am[k] += a[3 * j + k];
            bm[k] += b[3 * j + k];
        }
    for (int k = 0; k < 3; ++k) {
        am[k] /= (double)rows;
        bm[k] /= (double)rows;
    }
    double c[sim::kSums] = {};
    for (long long j = 0; j < rows; ++j)
        sim::add_centred(c, am, bm, a[3 * j], a[3 * j + 1], a[3 * j + 2], b[3 * j], b[3 * j + 1],
                         b[3 * j + 2]);
    return sim::fit(rows, am, bm, c, rigid, S);
}

int main(int argc, char** argv) {
    if (argc != 6) return 2;
    const long long rows = std::atoll(argv[3]);
    const bool rigid = std::atoi(argv[4]) != 0;
    const bool three = std::strcmp(argv[5], "3pt") == 0;
    if (rows < 1 || (three && rows != 3) || (!three && std::strcmp(argv[5], "fit") != 0)) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 3;
    std::vector<double> buf, rec(6 * rows);
    while (std::fread(rec.data(), sizeof(double), rec.size(), in) == rec.size())
        buf.insert(buf.end(), rec.begin(), rec.end());
    std::fclose(in);
    const size_t n = buf.size() / rec.size();
    std::vector<double> out(14 * n);
    for (size_t i = 0; i < n; ++i) {
        const double* a = &buf[6 * rows * i];
        double S[sim::kDoubles];
        const bool ok = three ? sim::similarity_3pt(a, a + 9, rigid, S)
                              : fit_rows(rows, a, a + 3 * rows, rigid, S);
        out[14 * i] = ok ? 1.0 : 0.0;
        for (int q = 0; q < sim::kDoubles; ++q) out[14 * i + 1 + q] = S[q];
    }
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 4;
    const bool ok = std::fwrite(out.data(), sizeof(double), out.size(), o) == out.size();
    std::fclose(o);
    return ok ? 0 : 5;
}
