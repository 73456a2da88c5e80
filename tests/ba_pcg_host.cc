// ba_pcg_host.cc -- openvslam_amd/csrc/ba_pcg_math.inc and ba_pcg_plan.inc through a plain host compiler (g++ -ffp-contract=off), for
// tests/test_ba_pcg_ref.py: whole solves with the device's lanes run one after the other, and the host plan. Built twice: plain, for the
// bits, and under AddressSanitizer + UndefinedBehaviorSanitizer, for the plan and the solver's edges.
//   ba_pcg_host solve in.bin out.bin
//       in:  n_cases, then per case n, tol, max_iter, S[n n] (row-major), g[n]       (flat doubles, counts as doubles too)
//       out: per case ok (1 / 0), x[n], info[3]
//   ba_pcg_host plan N_FREE TOL MAX_ITER CHECK_EVERY
//       prints "status n n_blocks max_iter check_every grid_product grid_update arena_bytes passes..." (the chunks' pass counts); after a
//       status other than 0 nothing else. Nothing is allocated.
//   ba_pcg_host edges
//       an indefinite matrix, a zero right-hand side, a non-positive diagonal block, a NaN: prints one line each, returns 0 when all
//       came out as rule P5 says.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string_view>
#include <vector>

#include "ba_pcg_math.inc"
#include "ba_pcg_plan.inc"

namespace {

std::vector<double> read_all(const char* path) {
    std::vector<double> v;
    FILE* f = std::fopen(path, "rb");
    if (!f) return v;
    double buf[512];
    size_t n;
    while ((n = std::fread(buf, 8, 512, f)) > 0) v.insert(v.end(), buf, buf + n);
    std::fclose(f);
    return v;
}

bool solve(const std::vector<double>& S, const std::vector<double>& g, int n, double tol, int max_iter, std::vector<double>& x, double* info) {
    pcgplan::Plan P;
    if (pcgplan::plan_of(n, tol, max_iter, 0, &P) != OVS_OK) return false;
    std::vector<double> work(pcg::solve_seq_work_doubles(n));
    x.assign((size_t)n, 0.0);
    return pcg::solve_seq(S.data(), (size_t)n, g.data(), n, tol, P.max_iter, x.data(), work.data(), info);
}

// a well-conditioned symmetric positive definite matrix: diagonally dominant
std::vector<double> spd(int n) {
    std::vector<double> S((size_t)n * n);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) S[(size_t)i * n + j] = i == j ? n + 1.0 : 1.0 / (1.0 + std::abs(i - j));
    return S;
}

int edges() {
    int bad = 0;
    const int n = 12;
    std::vector<double> x, g((size_t)n, 1.0);
    double info[3];
    {   // indefinite: positive definite diagonal blocks, a coupling that makes p.q negative
        std::vector<double> S((size_t)n * n, 0.0);
        for (int i = 0; i < n; ++i) S[(size_t)i * n + i] = 1.0;
        for (int i = 0; i < 6; ++i) S[(size_t)i * n + 6 + i] = S[(size_t)(6 + i) * n + i] = -3.0;
        for (int i = 0; i < n; ++i) g[i] = 1.0;   // p = g in the first pass: p.S p = 12 - 36 < 0
        const bool ok = solve(S, g, n, 1e-10, 0, x, info);
        std::printf("indefinite %d\n", ok ? 1 : 0);
        bad += ok ? 1 : 0;
    }
    {   // zero right-hand side: zero iterations, x = 0, no failure
        std::vector<double> S = spd(n), z((size_t)n, 0.0);
        const bool ok = solve(S, z, n, 1e-10, 0, x, info);
        bool zero = true;
        for (double v : x) zero = zero && v == 0.0;
        std::printf("zero_rhs %d %g %g %g %d\n", ok ? 1 : 0, info[0], info[1], info[2], zero ? 1 : 0);
        bad += (ok && zero && info[0] == 0.0 && info[1] == 0.0) ? 0 : 1;
    }
    {   // a diagonal block that is not positive definite
        std::vector<double> S = spd(n);
        S[(size_t)7 * n + 7] = -1.0;
        const bool ok = solve(S, g, n, 1e-10, 0, x, info);
        std::printf("bad_block %d\n", ok ? 1 : 0);
        bad += ok ? 1 : 0;
    }
    {   // a NaN off the diagonal blocks: p.q is not finite
        std::vector<double> S = spd(n);
        S[(size_t)1 * n + 8] = S[(size_t)8 * n + 1] = std::nan("");
        const bool ok = solve(S, g, n, 1e-10, 0, x, info);
        std::printf("nan %d\n", ok ? 1 : 0);
        bad += ok ? 1 : 0;
    }
    {   // the cap: three iterations of a system that needs more, reported and no failure
        const int m = 66;
        std::vector<double> S = spd(m), gm((size_t)m);
        for (int i = 0; i < m; ++i) gm[i] = 1.0 + i;
        const bool ok = solve(S, gm, m, 1e-10, 3, x, info);
        std::printf("cap %d %g %g\n", ok ? 1 : 0, info[0], info[1]);
        bad += (ok && info[0] == 3.0 && info[1] == 1.0) ? 0 : 1;
    }
    return bad;
}

}   // namespace

int main(int argc, char** argv) {
    if (argc == 2 && std::string_view(argv[1]) == "edges") return edges() == 0 ? 0 : 1;
    if (argc == 6 && std::string_view(argv[1]) == "plan") {
        pcgplan::Plan P;
        const long long nf = std::atoll(argv[2]);
        const ovs_status st = pcgplan::plan_of(6 * nf, std::atof(argv[3]), std::atoll(argv[4]), std::atoll(argv[5]), &P);
        std::printf("%d", (int)st);
        if (st == OVS_OK) {
            std::printf(" %d %d %d %d %d %d %zu", P.n, P.n_blocks, P.max_iter, P.check_every, P.grid_product, P.grid_update, P.arena_bytes);
            const size_t offs[11] = {P.o_L, P.o_x, P.o_r, P.o_z, P.o_p0, P.o_p1, P.o_q, P.o_pq, P.o_rz, P.o_scal, P.o_words};
            bool ordered = P.o_L == 0 && P.arena_bytes <= pcgplan::arena_bytes_max() && P.o_words + 4 * pcgplan::kWords <= P.arena_bytes;
            for (int i = 0; i + 1 < 11; ++i) ordered = ordered && offs[i] < offs[i + 1] && offs[i] % 256 == 0;
            std::printf(" %d", ordered ? 1 : 0);
            long long passes = 0;
            int chunks = 0;
            for (int first = 0;;) {
                const int c = pcgplan::chunk_passes(P, first);
                if (c == 0) break;
                first += c;
                passes += c;
                ++chunks;
            }
            std::printf(" %lld %d", passes, chunks);
        }
        std::printf("\n");
        return 0;
    }
    if (argc != 4 || std::string_view(argv[1]) != "solve") return 2;
    const std::vector<double> in = read_all(argv[2]);
    std::vector<double> out;
    size_t at = 0;
    const auto next = [&] { return at < in.size() ? in[at++] : 0.0; };
    const int n_cases = (int)next();
    for (int c = 0; c < n_cases; ++c) {
        const int n = (int)next();
        const double tol = next();
        const int max_iter = (int)next();
        if (n < 0 || (size_t)n * n + n > in.size() - at) return 5;
        std::vector<double> S(in.begin() + (long)at, in.begin() + (long)(at + (size_t)n * n));
        at += (size_t)n * n;
        std::vector<double> g(in.begin() + (long)at, in.begin() + (long)(at + n));
        at += (size_t)n;
        std::vector<double> x;
        double info[3] = {0, 0, 0};
        const bool ok = solve(S, g, n, tol, max_iter, x, info);
        x.resize((size_t)n, 0.0);
        out.push_back(ok ? 1.0 : 0.0);
        out.insert(out.end(), x.begin(), x.end());
        out.insert(out.end(), info, info + 3);
    }
    FILE* f = std::fopen(argv[3], "wb");
    if (!f) return 3;
    const bool ok = out.empty() || std::fwrite(out.data(), 8, out.size(), f) == out.size();
    return (std::fclose(f) == 0 && ok) ? 0 : 4;
}
