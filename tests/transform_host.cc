// The transform optimiser's algebra (openvslam_amd/csrc/sim3_opt_math.inc, include/ovs_detmath.h) run by a plain host compiler, the 64 lanes
// one after the other: tests/test_transform_ref.py builds this with g++ -ffp-contract=off and compares every double with the Python
// reference bit for bit. usage: transform_host in.bin out.bin
//
// in.bin (little endian): i32 n_det, n_det x {i32 fn (6 sin, 7 cos, 8 exp), f64 x}; i32 n_exp, n_exp x {f64 u[7], i32 fix_scale, f64 R[9], t[3], s};
// i32 n_problems, per problem {i32 n, fix_scale, num_iter, f32 chi_sq, 2 x {i32 model, f64 a b c d}, f64 R[9], t[3], s,
// n x {f64 p1[3] p2[3] obs1[2] obs2[2] w1 w2}}.
// out.bin: n_det f64; n_exp x f64 {R[9], t[3], s, s21, t21[3]}; per problem {i32 num_inliers, f64 R[9], t[3], s, info[8], n u8 outlier flags}.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sim3_opt_math.inc"

namespace {
struct Reader {
    const unsigned char *p, *end;
    template <typename T>
    T get() {
        if (p + sizeof(T) > end) {
            std::fprintf(stderr, "input too short\n");
            std::exit(2);
        }
        T v;
        std::memcpy(&v, p, sizeof(T));
        p += sizeof(T);
        return v;
    }
};

// the 64 lanes one after the other; rule 6's tree over their partial sums
struct HostLanes {
    static constexpr int kJacobianStride = 1;
    double J[28];
    double* jacobian(int) { return J; }
    template <class F>
    void each(F f) {
        for (int lane = 0; lane < 64; ++lane) f(lane);
    }
    template <int K, class F>
    void sum(F f, double (&out)[K]) {
        static double part[64][K];
        for (int j = 0; j < 64; ++j) {
            for (int k = 0; k < K; ++k) part[j][k] = 0.0;
            f(j, part[j]);
        }
        for (int d = 32; d; d >>= 1)
            for (int j = 0; j < d; ++j)
                for (int k = 0; k < K; ++k) part[j][k] = part[j][k] + part[j + d][k];
        for (int k = 0; k < K; ++k) out[k] = part[0][k];
    }
    template <class F>
    void count(F f, int (&out)[1]) {
        int c = 0;
        for (int lane = 0; lane < 64; ++lane) c += f(lane);
        out[0] = c;
    }
    void sync() {}
};

s3::Cam read_cam(Reader& r) {
    s3::Cam c;
    c.model = r.get<int32_t>();
    c.pad = 0;
    c.a = r.get<double>(), c.b = r.get<double>(), c.c = r.get<double>(), c.d = r.get<double>();
    return c;
}
void read_state(Reader& r, s3::State& S) {
    for (double& v : S.R) v = r.get<double>();
    for (double& v : S.t) v = r.get<double>();
    S.s = r.get<double>();
    s3::set_inverse(S);
}
void put(FILE* o, const double* v, size_t n) { std::fwrite(v, 8, n, o); }
}   // namespace

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::fseek(f, 0, SEEK_END);
    const long size = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    std::vector<unsigned char> buf((size_t)size);
    if (std::fread(buf.data(), 1, buf.size(), f) != buf.size()) return 2;
    std::fclose(f);
    Reader r{buf.data(), buf.data() + buf.size()};
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;

    for (int n = r.get<int32_t>(); n > 0; --n) {
        const int fn = r.get<int32_t>();
        const double x = r.get<double>();
        const double y = fn == 6 ? ovs_det_sin(x) : fn == 7 ? ovs_det_cos(x) : ovs_det_exp(x);
        put(o, &y, 1);
    }
    for (int n = r.get<int32_t>(); n > 0; --n) {
        double u[7];
        for (double& v : u) v = r.get<double>();
        const int fix = r.get<int32_t>();
        s3::State S, out;
        read_state(r, S);
        s3::exp_apply(u, fix, S, out);
        put(o, out.R, 9), put(o, out.t, 3), put(o, &out.s, 1), put(o, &out.s21, 1), put(o, out.t21, 3);
    }
    for (int np = r.get<int32_t>(); np > 0; --np) {
        const int n = r.get<int32_t>();
        s3::Params P;
        P.fix_scale = r.get<int32_t>();
        P.num_iter = r.get<int32_t>();
        const float chi_sq = r.get<float>();
        P.chi_sq = (double)chi_sq;
        P.delta = (double)std::sqrt(chi_sq);
        P.delta_sq = P.delta * P.delta;
        const s3::Cam cam1 = read_cam(r), cam2 = read_cam(r);
        s3::State S;
        read_state(r, S);
        std::vector<s3::Match> ms((size_t)n);
        for (s3::Match& m : ms) {
            for (double& v : m.p1) v = r.get<double>();
            for (double& v : m.p2) v = r.get<double>();
            for (double& v : m.o1) v = r.get<double>();
            for (double& v : m.o2) v = r.get<double>();
            m.w1 = r.get<double>(), m.w2 = r.get<double>();
        }
        std::vector<uint8_t> outlier((size_t)n + 1);
        s3::State pert[14];
        s3::Result res;
        HostLanes x;
        s3::s3_optimize(x, cam1, cam2, n, [&](int i) { return ms[(size_t)i]; }, S, P, outlier.data(), pert, res);
        const int32_t num = res.num_inliers;
        std::fwrite(&num, 4, 1, o);
        put(o, res.est.R, 9), put(o, res.est.t, 3), put(o, &res.est.s, 1), put(o, res.info, 8);
        std::fwrite(outlier.data(), 1, (size_t)n, o);
    }
    std::fclose(o);
    return 0;
}
