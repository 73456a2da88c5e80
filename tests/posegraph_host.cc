// posegraph_host.cc -- openvslam_amd/csrc/pose_graph_math.inc through a plain host compiler (g++ -ffp-contract=off), for
// tests/test_posegraph_ref.py: ovs_det_log on a grid, the Sim3 logarithm on given states and whole optimisations, with the lanes of
// the device run one after the other. Input and output are flat arrays of doubles (counts and indices as doubles too):
//   in:  n_log, x[n_log]; n_states, (R 9, t 3, s)[n_states]; n_scenes, then per scene n_v, n_e, n_l, fix_scale, num_iter, pcg_max_iter,
//        V[13 n_v], nc[13 n_v], fixed[n_v], edge_ij[2 n_e], meas[13 n_e], lm_ref[n_l], lm_pos[3 n_l]
//   out: det_log(x)[n_log]; log[7 n_states]; per scene V[13 n_v], lm[3 n_l], info[8]
// usage: posegraph_host in.bin out.bin
#include <cstdio>
#include <vector>

#include "pose_graph_math.inc"
#include "pose_graph_plan.inc"

namespace {

struct HostLanes {
    static constexpr int kLanes = 256;
    template <class F>
    void each(F f) {
        for (int lane = 0; lane < kLanes; ++lane) f(lane);
    }
    void sync() {}
    double sum(int n, const double* val, const uint8_t* skip) {
        double part[64];
        for (int j = 0; j < 64; ++j) {
            part[j] = 0.0;
            for (int i = j; i < n; i += 64)
                if (!skip || !skip[i]) part[j] = part[j] + val[i];
        }
        for (int d = 32; d; d >>= 1)
            for (int j = 0; j < d; ++j) part[j] = part[j] + part[j + d];
        return part[0];
    }
};

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

}   // namespace

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    const std::vector<double> in = read_all(argv[1]);
    std::vector<double> out;
    size_t at = 0;
    const auto next = [&] { return at < in.size() ? in[at++] : 0.0; };
    const int n_log = (int)next();
    for (int k = 0; k < n_log; ++k) out.push_back(ovs_det_log(next()));
    const int n_states = (int)next();
    for (int k = 0; k < n_states; ++k) {
        double rec[13], e[7];
        for (double& x : rec) x = next();
        pg::log_of(pg::load_state(rec), e);
        out.insert(out.end(), e, e + 7);
    }
    const int n_scenes = (int)next();
    for (int k = 0; k < n_scenes; ++k) {
        const int n_v = (int)next(), n_e = (int)next(), n_l = (int)next();
        pg::Params prm;
        prm.fix_scale = (int)next(), prm.num_iter = (int)next(), prm.pcg_max_iter = (int)next();
        std::vector<double> V(13 * (size_t)n_v + 1), nc(13 * (size_t)n_v + 1), meas(13 * (size_t)n_e + 1), lm_pos(3 * (size_t)n_l + 1);
        std::vector<uint8_t> fixed((size_t)n_v + 1);
        std::vector<int32_t> edge_ij(2 * (size_t)n_e + 1), lm_ref((size_t)n_l + 1), inc_row((size_t)n_v + 1), inc(2 * (size_t)n_e + 1);
        for (int i = 0; i < 13 * n_v; ++i) V[i] = next();
        for (int i = 0; i < 13 * n_v; ++i) nc[i] = next();
        for (int i = 0; i < n_v; ++i) fixed[i] = (uint8_t)next();
        for (int i = 0; i < 2 * n_e; ++i) edge_ij[i] = (int32_t)next();
        for (int i = 0; i < 13 * n_e; ++i) meas[i] = next();
        for (int i = 0; i < n_l; ++i) lm_ref[i] = (int32_t)next();
        for (int i = 0; i < 3 * n_l; ++i) lm_pos[i] = next();
        std::vector<double> Vt(V.size()), edge((size_t)pg::kEdgeDoubles * n_e + 1), chi_e((size_t)n_e + 1), Hd(49 * (size_t)n_v + 1), Lf(Hd.size()),
            g(7 * (size_t)n_v + 1), x(g.size()), r(g.size()), z(g.size()), p(g.size()), q(g.size()), val((size_t)n_v + 1);
        pg::Problem P;
        P.n_v = n_v, P.n_e = n_e;
        P.n_free = pgplan::build_incidence(n_v, n_e, edge_ij.data(), fixed.data(), inc_row.data(), inc.data());
        P.fixed = fixed.data(), P.edge_ij = edge_ij.data(), P.meas = meas.data(), P.inc_row = inc_row.data(), P.inc = inc.data();
        P.V = V.data(), P.Vt = Vt.data(), P.edge = edge.data(), P.chi_e = chi_e.data(), P.Hd = Hd.data(), P.Lf = Lf.data();
        P.g = g.data(), P.x = x.data(), P.r = r.data(), P.z = z.data(), P.p = p.data(), P.q = q.data(), P.val = val.data();
        HostLanes lanes;
        double info[8];
        pg::pg_optimize(lanes, P, prm, info);
        out.insert(out.end(), V.begin(), V.begin() + 13 * n_v);
        for (int m = 0; m < n_l; ++m) {
            double c[3] = {lm_pos[3 * m], lm_pos[3 * m + 1], lm_pos[3 * m + 2]};
            if (lm_ref[m] >= 0)
                pg::correct_landmark(pg::load_state(nc.data() + 13 * (size_t)lm_ref[m]), pg::load_state(V.data() + 13 * (size_t)lm_ref[m]), lm_pos.data() + 3 * m, c);
            out.insert(out.end(), c, c + 3);
        }
        out.insert(out.end(), info, info + 8);
    }
    FILE* f = std::fopen(argv[2], "wb");
    if (!f) return 3;
    const bool ok = out.empty() || std::fwrite(out.data(), 8, out.size(), f) == out.size();
    return (std::fclose(f) == 0 && ok) ? 0 : 4;
}
