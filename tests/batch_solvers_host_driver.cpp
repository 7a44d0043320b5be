// Host build of csrc/batch_solvers.hpp (the code the batched solvers' kernels
// run) beside lm_core.hpp, which it is checked against:
//   batch_solvers_host_driver chol P IN OUT
//     IN: systems of P*P + P doubles (A row-major, full; b).  OUT per system
//     2 (1 + P) doubles: chol_ut<P>'s flag and x, then lm::cholesky_solve's
//     (x starts as zeros in both, so a failure leaves the same bytes).
//   batch_solvers_host_driver lm IN OUT
//     IN: problems [P, kind, M, max_it, ctol, ptol, gtol, mu0, x0[P], T[M*P],
//     y[M]]: residuals r_i = exp(T_i . x) - y_i; kind 1: every point but x0
//     evaluates to NaN.  OUT per problem two records (the pieces, then
//     lm_core.hpp's start / consume / advance) of kRec doubles:
//     [evaluations, iterations, stop class (1 tolerance, 2 failed, 0
//     iterations), rejected trials, Cholesky retries, x[9], xn[kMaxEval][9]].
//   batch_solvers_host_driver gain IN OUT
//     IN: rows [F, Fn, pred, comparable, mu, nu].  OUT per row [rho, the
//     value gain_update returns, mu, nu after it].
//   batch_solvers_host_driver order IN OUT
//     IN: N keys [count, score, h, k].  OUT: N*N bytes better(key i, key j).
//   batch_solvers_host_driver tree IN OUT
//     IN: arrangements of 256 keys.  OUT per arrangement 8 doubles: the
//     winner of the kernels' pairwise tree, then of a sequential scan.
//   batch_solvers_host_driver draw SEED DRAWS CNT H OUT
//     OUT: H*DRAWS int64: ransac::draw(seed, h, d, DRAWS, CNT).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lm_core.hpp"  // includes batch_solvers.hpp

using namespace acm;

static std::vector<double> read_all(const char* path) {
    std::vector<double> buf;
    FILE* in = std::fopen(path, "rb");
    if (!in) std::exit(3);
    double chunk[4096];
    size_t got;
    while ((got = std::fread(chunk, sizeof(double), 4096, in)) > 0)
        buf.insert(buf.end(), chunk, chunk + got);
    std::fclose(in);
    return buf;
}

static int write_all(const char* path, const void* p, size_t bytes) {
    FILE* o = std::fopen(path, "wb");
    if (!o) return 4;
    const bool ok = std::fwrite(p, 1, bytes, o) == bytes;
    std::fclose(o);
    return ok ? 0 : 5;
}

template <int P>
static void chol_both(const std::vector<double>& in, std::vector<double>& out) {
    const size_t rec = P * P + P, n = in.size() / rec;
    out.assign(n * 2 * (1 + P), 0.0);
    for (size_t i = 0; i < n; ++i) {
        const double* A = &in[rec * i];
        const double* b = A + P * P;
        double Au[P * (P + 1) / 2];
        for (int r = 0; r < P; ++r)
            for (int q = r; q < P; ++q) Au[ut<P>(r, q)] = A[r * P + q];
        double* o = &out[i * 2 * (1 + P)];
        o[0] = chol_ut<P>(Au, b, o + 1) ? 1.0 : 0.0;
        o[1 + P] = lm::cholesky_solve(P, A, b, o + 2 + P) ? 1.0 : 0.0;
    }
}

constexpr int kMaxEval = 64;
constexpr int kRec = 5 + 9 + 9 * kMaxEval;

struct Problem {
    int P, kind, M, max_it;
    double ctol, ptol, gtol, mu0;
    const double *x0, *T, *y;
};

// res = [J^T J (P x P) | J^T r | 0.5 r.r | n], acm_normal_equations' layout
static void evaluate(const Problem& p, const double* x, double* res) {
    const int P = p.P;
    for (int i = 0; i < P * P + P + 2; ++i) res[i] = 0.0;
    bool at_start = true;
    for (int k = 0; k < P; ++k) at_start = at_start && x[k] == p.x0[k];
    double rr = 0.0;
    for (int i = 0; i < p.M; ++i) {
        double s = 0.0;
        for (int k = 0; k < P; ++k) s += p.T[i * P + k] * x[k];
        const double e = exp(s);
        double r = e - p.y[i];
        if (p.kind == 1 && !at_start) r = NAN;
        for (int a = 0; a < P; ++a) {
            for (int b = 0; b < P; ++b) res[a * P + b] += (e * p.T[i * P + a]) * (e * p.T[i * P + b]);
            res[P * P + a] += (e * p.T[i * P + a]) * r;
        }
        rr += r * r;
    }
    res[P * P + P] = 0.5 * rr;
    res[P * P + P + 1] = p.M;
}

static void record_eval(double* rec, int n, const double* xn, int P) {
    if (n < kMaxEval)
        for (int k = 0; k < P; ++k) rec[14 + 9 * n + k] = xn[k];
}

// the loop k_triangulate and k_pose_batch build from the pieces
template <int P>
static void run_pieces(const Problem& p, double* rec) {
    constexpr int T = P * (P + 1) / 2;
    double x[P], xn[P], h[P], A[T], g[P], res[P * P + P + 2];
    for (int k = 0; k < P; ++k) {
        x[k] = xn[k] = p.x0[k];
        h[k] = g[k] = 0.0;
    }
    for (int k = 0; k < T; ++k) A[k] = 0.0;
    double F = 0.0, mu = 0.0, nu = 2.0, dmax = 0.0;
    int it = 0, term = 0, evals = 0, rejected = 0, retries = 0;
    bool first = true;
    for (;;) {
        evaluate(p, xn, res);
        record_eval(rec, evals++, xn, P);
        double An[T];
        for (int r = 0; r < P; ++r)
            for (int q = r; q < P; ++q) An[ut<P>(r, q)] = res[r * P + q];
        const double* gn = res + P * P;
        const double Fn = res[P * P + P];
        bool accept = false;
        if (first) {
            first = false;
            accept = true;
            for (int k = 0; k < P; ++k) dmax = fmax(dmax, An[ut<P>(k, k)]);
            mu = p.mu0;
            nu = 2.0;
            if (!__builtin_isfinite(Fn)) term = 2;
        } else {
            const double pred = lm::predicted_reduction<P>(A, g, h);
            const int gain = lm::gain_update(lm::gain_ratio(F, Fn, pred, true), mu, nu);
            accept = gain == lm::GAIN_ACCEPT;
            if (!accept) ++rejected;
            if (gain == lm::GAIN_FAILED) term = 2;
        }
        if (accept) {
            const double dF = F - Fn, Fold = F;
            const bool trial = it > 0;
            for (int k = 0; k < P; ++k) x[k] = xn[k];
            for (int k = 0; k < T; ++k) A[k] = An[k];
            for (int k = 0; k < P; ++k) g[k] = gn[k];
            F = Fn;
            if (term == 0 && lm::accepted_terminates<P>(g, p.gtol, trial, dF, Fold, p.ctol)) term = 1;
        }
        if (term != 0) break;
        const int before = it;
        const int step = lm::next_step<P>(A, g, x, mu, nu, dmax, p.ptol, it, p.max_it, xn, h);
        retries += it - before - (step == lm::STEP_EXHAUSTED ? 0 : 1);
        if (step == lm::STEP_CONVERGED) term = 1;
        if (step != lm::STEP_EVALUATE) break;
    }
    rec[0] = evals;
    rec[1] = it;
    rec[2] = term;
    rec[3] = rejected;
    rec[4] = retries;
    for (int k = 0; k < P; ++k) rec[5 + k] = x[k];
}

static void run_lm_core(const Problem& p, double* rec) {
    acm_lm_config cfg;
    std::memset(&cfg, 0, sizeof(cfg));
    cfg.max_iterations = p.max_it;
    cfg.cost_tolerance = p.ctol;
    cfg.parameter_tolerance = p.ptol;
    cfg.gradient_tolerance = p.gtol;
    cfg.initial_damping = p.mu0;
    cfg.has_bounds = 0;
    lm::State s;
    lm::start(s, cfg, p.P, p.x0);
    double res[9 * 9 + 9 + 2];
    int evals = 0;
    for (;;) {
        evaluate(p, s.xn, res);
        record_eval(rec, evals++, s.xn, p.P);
        if (lm::consume(s, cfg, res, p.P) == lm::DONE) break;
    }
    rec[0] = evals;
    rec[1] = s.it;
    rec[2] = s.term == ACM_LM_MAX_ITERATIONS ? 0 : (s.term == ACM_LM_FAILED ? 2 : 1);
    for (int k = 0; k < p.P; ++k) rec[5 + k] = s.x[k];
}

static int mode_lm(const char* in_path, const char* out_path) {
    const std::vector<double> in = read_all(in_path);
    std::vector<double> out;
    size_t at = 0;
    while (at + 8 <= in.size()) {
        Problem p;
        p.P = (int)in[at];
        p.kind = (int)in[at + 1];
        p.M = (int)in[at + 2];
        p.max_it = (int)in[at + 3];
        p.ctol = in[at + 4];
        p.ptol = in[at + 5];
        p.gtol = in[at + 6];
        p.mu0 = in[at + 7];
        const size_t need = 8 + (size_t)p.P + (size_t)p.M * p.P + p.M;
        if ((p.P != 3 && p.P != 6) || p.M < 1 || p.max_it < 1 || p.max_it >= kMaxEval ||
            at + need > in.size())
            return 2;
        p.x0 = &in[at + 8];
        p.T = p.x0 + p.P;
        p.y = p.T + (size_t)p.M * p.P;
        at += need;
        out.resize(out.size() + 2 * kRec, 0.0);
        double* rec = &out[out.size() - 2 * kRec];
        if (p.P == 3) run_pieces<3>(p, rec);
        else run_pieces<6>(p, rec);
        run_lm_core(p, rec + kRec);
    }
    return write_all(out_path, out.data(), out.size() * sizeof(double));
}

static int mode_gain(const char* in_path, const char* out_path) {
    const std::vector<double> in = read_all(in_path);
    const size_t n = in.size() / 6;
    std::vector<double> out(4 * n);
    for (size_t i = 0; i < n; ++i) {
        const double* r = &in[6 * i];
        double mu = r[4], nu = r[5];
        const double rho = lm::gain_ratio(r[0], r[1], r[2], r[3] != 0.0);
        out[4 * i] = rho;
        out[4 * i + 1] = lm::gain_update(rho, mu, nu);
        out[4 * i + 2] = mu;
        out[4 * i + 3] = nu;
    }
    return write_all(out_path, out.data(), out.size() * sizeof(double));
}

static ransac::Key key_at(const double* k) {
    return ransac::Key{(int)k[0], k[1], (int)k[2], (int)k[3]};
}

static int mode_order(const char* in_path, const char* out_path) {
    const std::vector<double> in = read_all(in_path);
    const size_t n = in.size() / 4;
    std::vector<unsigned char> out(n * n);
    for (size_t i = 0; i < n; ++i)
        for (size_t j = 0; j < n; ++j)
            out[i * n + j] = ransac::better(key_at(&in[4 * i]), key_at(&in[4 * j])) ? 1 : 0;
    return write_all(out_path, out.data(), out.size());
}

static int mode_tree(const char* in_path, const char* out_path) {
    const std::vector<double> in = read_all(in_path);
    const size_t n = in.size() / (4 * 256);
    std::vector<double> out(8 * n);
    for (size_t a = 0; a < n; ++a) {
        ransac::Key key[256];
        for (int t = 0; t < 256; ++t) key[t] = key_at(&in[4 * (256 * a + t)]);
        ransac::Key scan = key[0];
        for (int t = 1; t < 256; ++t)
            if (ransac::better(key[t], scan)) scan = key[t];
        // the workgroup's tree: thread t < off takes slot t + off when it is better
        for (int off = 128; off > 0; off >>= 1)
            for (int t = 0; t < off; ++t)
                if (ransac::better(key[t + off], key[t])) key[t] = key[t + off];
        const ransac::Key w[2] = {key[0], scan};
        for (int q = 0; q < 2; ++q) {
            out[8 * a + 4 * q] = w[q].count;
            out[8 * a + 4 * q + 1] = w[q].score;
            out[8 * a + 4 * q + 2] = w[q].h;
            out[8 * a + 4 * q + 3] = w[q].k;
        }
    }
    return write_all(out_path, out.data(), out.size() * sizeof(double));
}

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const char* mode = argv[1];
    if (!std::strcmp(mode, "chol") && argc == 5) {
        const int P = std::atoi(argv[2]);
        const std::vector<double> in = read_all(argv[3]);
        std::vector<double> out;
        if (P == 3) chol_both<3>(in, out);
        else if (P == 6) chol_both<6>(in, out);
        else if (P == 9) chol_both<9>(in, out);
        else return 2;
        return write_all(argv[4], out.data(), out.size() * sizeof(double));
    }
    if (!std::strcmp(mode, "lm") && argc == 4) return mode_lm(argv[2], argv[3]);
    if (!std::strcmp(mode, "gain") && argc == 4) return mode_gain(argv[2], argv[3]);
    if (!std::strcmp(mode, "order") && argc == 4) return mode_order(argv[2], argv[3]);
    if (!std::strcmp(mode, "tree") && argc == 4) return mode_tree(argv[2], argv[3]);
    if (!std::strcmp(mode, "draw") && argc == 7) {
        const unsigned long long seed = std::strtoull(argv[2], nullptr, 10);
        const int draws = std::atoi(argv[3]), H = std::atoi(argv[5]);
        const long long cnt = std::atoll(argv[4]);
        if (draws < 1 || H < 1 || cnt < 1) return 2;
        std::vector<long long> out((size_t)H * draws);
        for (int h = 0; h < H; ++h)
            for (int d = 0; d < draws; ++d) out[(size_t)h * draws + d] = ransac::draw(seed, h, d, draws, cnt);
        return write_all(argv[6], out.data(), out.size() * sizeof(long long));
    }
    return 2;
}
