// The batch solvers' host plan (openvslam_amd/csrc/solve_plan.inc) as a stand-alone host program: no device, no library, the plain host compiler.
// It reads rows on stdin and prints one line per row, read by tests/test_solve_plan.py. A row is KIND:FAMILY[:key=value]...; FAMILY is one of
// sim3 pnp sim3opt twoview essential reconstruct triangulate landmarks.
//   layout:FAMILY:P=..:T=..[:desc=1]   ->  every section offset of the Layout in its declaration order (for landmarks: ... total bytes)
//   check:FAMILY:...                   ->  status T run        (the family's check; the keys and their defaults are below)
//   stage:FAMILY:...                   ->  bytes, then the staged block in hexadecimal (a heap buffer of exactly `bytes`, 0xee where nothing was
//                                          written); for triangulate and landmarks then the caller's arrays after collect, one hexadecimal
//                                          field each, on output sections filled with out_pattern; for landmarks before them n8, n64 and the
//                                          keyframe table
// Keys of every family: h (1: the call has a handle), maxp, maxt (its capacities), P, off (the offsets, comma-separated, or - for NULL), null (the
// names of the Call's pointers to pass as NULL, joined by +), and the family's scalars by the Call's names; cam1 / cam2: the camera of every problem
// on that side, by name (cameras()). Input array number `id` holds id * 16 + i at element i, in the Call's order of arrays.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <limits>
#include <map>
#include <string>
#include <vector>

#include "solve_plan.inc"

namespace {

using Args = std::map<std::string, std::string>;

bool g_bad = false;

std::vector<std::string> split(const std::string& row, char sep) {
    std::vector<std::string> v(1);
    for (const char c : row) {
        if (c == sep) v.emplace_back();
        else v.back().push_back(c);
    }
    return v;
}
double real(const std::string& s) {
    char* end = nullptr;
    const double x = std::strtod(s.c_str(), &end);
    if (s.empty() || *end) g_bad = true;
    return x;
}
int32_t integer(const std::string& s) {
    char* end = nullptr;
    const long long x = std::strtoll(s.c_str(), &end, 10);
    if (s.empty() || *end) g_bad = true;
    return (int32_t)x;
}
std::string get(const Args& a, const char* key, const char* dflt) {
    const auto it = a.find(key);
    return it == a.end() ? std::string(dflt) : it->second;
}
int32_t geti(const Args& a, const char* key, int32_t dflt) {
    const auto it = a.find(key);
    return it == a.end() ? dflt : integer(it->second);
}
double getd(const Args& a, const char* key, double dflt) {
    const auto it = a.find(key);
    return it == a.end() ? dflt : real(it->second);
}
std::vector<int32_t> ints(const std::string& s) {
    std::vector<int32_t> v;
    if (s.empty()) return v;
    for (const std::string& t : split(s, ',')) v.push_back(integer(t));
    return v;
}
bool wants_null(const Args& a, const char* name) {
    for (const std::string& t : split(get(a, "null", ""), '+'))
        if (t == name) return true;
    return false;
}

template <class T>
std::vector<T> pattern(size_t n, int id) {
    std::vector<T> v(n ? n : 1);
    for (size_t i = 0; i < n; ++i) v[i] = (T)(id * 16 + (int)i);
    return v;
}
void out_pattern(uint8_t* at, size_t n, int id) {
    for (size_t i = 0; i < n; ++i) at[i] = (uint8_t)(id * 40 + (int)i);
}
void hex(const void* p, size_t n) {
    const uint8_t* b = static_cast<const uint8_t*>(p);
    std::printf(" ");
    if (n == 0) std::printf("-");
    for (size_t i = 0; i < n; ++i) std::printf("%02x", b[i]);
}

ovs_camera camera(const std::string& name, int p) {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    ovs_camera c{};
    c.model = 0, c.setup = 0;
    c.fx = 458.0 + p, c.fy = 457.0 + p, c.cx = 367.0 + p, c.cy = 248.0 + p;
    c.focal_x_baseline = 40.0 + p, c.true_baseline = 0.5 + p;
    c.cols = 752, c.rows = 480;
    if (name == "ok") return c;
    if (name == "equi") c.model = 1, c.cols = 1920 + p, c.rows = 960 + p;
    else if (name == "model2") c.model = 2;
    else if (name == "nanfx") c.fx = nan;
    else if (name == "inffy") c.fy = inf;
    else if (name == "nancx") c.cx = nan;
    else if (name == "infcy") c.cy = inf;
    else if (name == "fx0") c.fx = 0.0;
    else if (name == "fy0") c.fy = 0.0;
    else if (name == "norows") c.model = 1, c.cols = 1920, c.rows = 0;
    else if (name == "nocols") c.model = 1, c.cols = 0, c.rows = 960;
    else g_bad = true;
    return c;
}
std::vector<ovs_camera> cameras(const std::string& name, int n) {
    std::vector<ovs_camera> v((size_t)(n > 0 ? n : 1));
    for (int p = 0; p < n; ++p) v[(size_t)p] = camera(name, p);
    return v;
}

// what every family's row has in common
struct Common {
    bool handle;
    int32_t maxp, maxt, P, T;
    std::vector<int32_t> off;
    const int32_t* offsets;
    size_t np, nt;   // elements to give the per-problem and per-match arrays
    explicit Common(const Args& a) {
        handle = geti(a, "h", 1) != 0;
        maxp = geti(a, "maxp", 2), maxt = geti(a, "maxt", 70), P = geti(a, "P", 1);
        const std::string o = get(a, "off", "0,65");
        if (o != "-") off = ints(o);
        offsets = o == "-" ? nullptr : off.data();
        if (offsets && P >= 0 && off.size() != (size_t)P + 1) g_bad = true;
        T = off.empty() ? 0 : off.back();
        np = (size_t)(maxp > P ? maxp : P > 0 ? P : 1);
        nt = (size_t)(maxt > T ? maxt : T > 0 ? T : 1);
    }
};

void print(const splan::Checked& k) { std::printf("%d %d %d\n", (int)k.status, (int)k.T, k.run ? 1 : 0); }

// the staged block on the heap, exactly `bytes` long
struct Block {
    uint8_t* p;
    size_t bytes;
    explicit Block(size_t n) : p(static_cast<uint8_t*>(std::malloc(n ? n : 1))), bytes(n) { std::memset(p, 0xee, n); }
    ~Block() { std::free(p); }
    Block(const Block&) = delete;
    Block& operator=(const Block&) = delete;
};

#define NUL(field) (wants_null(a, #field) ? (void)(c.field = nullptr) : (void)0)

bool run_sim3(const std::string& kind, const Args& a) {
    namespace F = splan::sim3;
    const Common m(a);
    const auto p1 = pattern<double>(3 * m.nt, 1), p2 = pattern<double>(3 * m.nt, 2);
    const auto thr1 = pattern<float>(m.nt, 3), thr2 = pattern<float>(m.nt, 4);
    const auto cams_1 = cameras(get(a, "cam1", "ok"), (int)m.np), cams_2 = cameras(get(a, "cam2", "equi"), (int)m.np);
    std::vector<int32_t> oi(3 * m.np);
    std::vector<double> od(13 * m.np);
    std::vector<uint8_t> of(m.nt);
    F::Call c{m.handle, m.P, m.offsets, p1.data(), p2.data(), thr1.data(), thr2.data(), cams_1.data(), cams_2.data(), geti(a, "min_num_inliers", 20),
              geti(a, "max_num_iter", 200), oi.data(), oi.data() + m.np, oi.data() + 2 * m.np, od.data(), od.data() + 9 * m.np, od.data() + 12 * m.np,
              of.data()};
    NUL(p1), NUL(p2), NUL(thr1), NUL(thr2), NUL(cams_1), NUL(cams_2), NUL(out_valid), NUL(out_best_iter), NUL(out_num_inliers), NUL(out_rot),
        NUL(out_trans), NUL(out_scale), NUL(out_flags);
    if (g_bad) return false;
    const splan::Checked k = F::check(c, [&] { return splan::Caps{m.maxp, m.maxt, 0, 0}; });
    if (kind == "check") return print(k), true;
    if (!k.run) return false;
    const F::Layout lay = F::layout_of(m.P, k.T);
    Block b(lay.bytes);
    F::stage(c, lay, b.p);
    std::printf("%zu", lay.bytes), hex(b.p, b.bytes), std::printf("\n");
    return true;
}

bool run_pnp(const std::string& kind, const Args& a) {
    namespace F = splan::pnp;
    const Common m(a);
    const auto bearings = pattern<double>(3 * m.nt, 1), pos_w = pattern<double>(3 * m.nt, 2), max_cos = pattern<double>(m.nt, 3);
    std::vector<int32_t> oi(3 * m.np);
    std::vector<double> od(12 * m.np);
    std::vector<uint8_t> of(m.nt);
    F::Call c{m.handle, m.P, m.offsets, bearings.data(), pos_w.data(), max_cos.data(), geti(a, "min_num_inliers", 10), geti(a, "max_num_iter", 200),
              oi.data(), oi.data() + m.np, oi.data() + 2 * m.np, od.data(), od.data() + 9 * m.np, of.data()};
    NUL(bearings), NUL(pos_w), NUL(max_cos_errors), NUL(out_valid), NUL(out_best_iter), NUL(out_num_inliers), NUL(out_rot), NUL(out_trans), NUL(out_flags);
    if (g_bad) return false;
    const splan::Checked k = F::check(c, [&] { return splan::Caps{m.maxp, m.maxt, 0, 0}; });
    if (kind == "check") return print(k), true;
    if (!k.run) return false;
    const F::Layout lay = F::layout_of(m.P, k.T);
    Block b(lay.bytes);
    F::stage(c, lay, b.p);
    std::printf("%zu", lay.bytes), hex(b.p, b.bytes), std::printf("\n");
    return true;
}

bool run_sim3opt(const std::string& kind, const Args& a) {
    namespace F = splan::sim3opt;
    const Common m(a);
    const auto p1 = pattern<double>(3 * m.nt, 1), p2 = pattern<double>(3 * m.nt, 2), obs1 = pattern<double>(2 * m.nt, 3), obs2 = pattern<double>(2 * m.nt, 4);
    const auto w1 = pattern<float>(m.nt, 5), w2 = pattern<float>(m.nt, 6);
    const auto cams_1 = cameras(get(a, "cam1", "ok"), (int)m.np), cams_2 = cameras(get(a, "cam2", "equi"), (int)m.np);
    const auto rot = pattern<double>(9 * m.np, 7), trans = pattern<double>(3 * m.np, 8), scale = pattern<double>(m.np, 9);
    std::vector<int32_t> oi(m.np);
    std::vector<double> od(13 * m.np);
    std::vector<uint8_t> of(m.nt);
    F::Call c{m.handle, m.P, m.offsets, p1.data(), p2.data(), obs1.data(), obs2.data(), w1.data(), w2.data(), cams_1.data(), cams_2.data(), rot.data(),
              trans.data(), scale.data(), (float)getd(a, "chi_sq", 10.0), geti(a, "num_iter", 10), oi.data(), od.data(), od.data() + 9 * m.np,
              od.data() + 12 * m.np, of.data()};
    NUL(p1), NUL(p2), NUL(obs1), NUL(obs2), NUL(inv_sigma_sq_1), NUL(inv_sigma_sq_2), NUL(cams_1), NUL(cams_2), NUL(rot_12_in), NUL(trans_12_in),
        NUL(scale_12_in), NUL(out_num_inliers), NUL(out_rot), NUL(out_trans), NUL(out_scale), NUL(out_flags);
    if (g_bad) return false;
    const splan::Checked k = F::check(c, [&] { return splan::Caps{m.maxp, m.maxt, 0, 0}; });
    if (kind == "check") return print(k), true;
    if (!k.run) return false;
    const F::Layout lay = F::layout_of(m.P, k.T);
    Block b(lay.bytes);
    F::stage(c, lay, b.p);
    std::printf("%zu", lay.bytes), hex(b.p, b.bytes), std::printf("\n");
    return true;
}

bool run_twoview(const std::string& kind, const Args& a) {
    namespace F = splan::twoview;
    const Common m(a);
    const auto x1 = pattern<double>(2 * m.nt, 1), x2 = pattern<double>(2 * m.nt, 2);
    std::vector<int32_t> oi(7 * m.np);
    std::vector<double> od(20 * m.np);
    std::vector<uint8_t> of(2 * m.nt);
    F::Call c{m.handle, m.P, m.offsets, x1.data(), x2.data(), getd(a, "sigma", 1.0), geti(a, "max_num_iter", 200), geti(a, "models", 3), od.data(),
              od.data() + 9 * m.np, od.data() + 18 * m.np, oi.data(), oi.data() + 2 * m.np, oi.data() + 4 * m.np, oi.data() + 6 * m.np, of.data(),
              of.data() + m.nt};
    NUL(x1), NUL(x2), NUL(out_H_21), NUL(out_F_21), NUL(out_scores), NUL(out_valid), NUL(out_best_iter), NUL(out_num_inliers), NUL(out_selected),
        NUL(out_flags_H), NUL(out_flags_F);
    if (g_bad) return false;
    const splan::Checked k = F::check(c, [&] { return splan::Caps{m.maxp, m.maxt, 0, 0}; });
    if (kind == "check") return print(k), true;
    if (!k.run) return false;
    const F::Layout lay = F::layout_of(m.P, k.T);
    Block b(lay.bytes);
    F::stage(c, lay, b.p);
    std::printf("%zu", lay.bytes), hex(b.p, b.bytes), std::printf("\n");
    return true;
}

bool run_essential(const std::string& kind, const Args& a) {
    namespace F = splan::essential;
    const Common m(a);
    const auto b1 = pattern<double>(3 * m.nt, 1), b2 = pattern<double>(3 * m.nt, 2);
    std::vector<int32_t> oi(3 * m.np);
    std::vector<double> od(10 * m.np);
    std::vector<uint8_t> of(m.nt);
    F::Call c{m.handle, m.P, m.offsets, b1.data(), b2.data(), getd(a, "residual_cos_thr", 0.01), geti(a, "max_num_iter", 200), od.data(),
              od.data() + 9 * m.np, oi.data(), oi.data() + m.np, oi.data() + 2 * m.np, of.data()};
    NUL(bearings_1), NUL(bearings_2), NUL(out_E_21), NUL(out_scores), NUL(out_valid), NUL(out_best_iter), NUL(out_num_inliers), NUL(out_flags);
    if (g_bad) return false;
    const splan::Checked k = F::check(c, [&] { return splan::Caps{m.maxp, m.maxt, 0, 0}; });
    if (kind == "check") return print(k), true;
    if (!k.run) return false;
    const F::Layout lay = F::layout_of(m.P, k.T);
    Block b(lay.bytes);
    F::stage(c, lay, b.p);
    std::printf("%zu", lay.bytes), hex(b.p, b.bytes), std::printf("\n");
    return true;
}

bool run_reconstruct(const std::string& kind, const Args& a) {
    namespace F = splan::reconstruct;
    const Common m(a);
    std::vector<int32_t> models = ints(get(a, "models", ""));
    for (size_t p = models.size(); p < m.np; ++p) models.push_back(1 + (int32_t)(p % 2));
    const auto mats = pattern<double>(9 * m.np, 1);
    const auto cams = cameras(get(a, "cam1", "ok"), (int)m.np);
    const auto inlier = pattern<uint8_t>(m.nt, 2);
    const auto kp_ref = pattern<double>(2 * m.nt, 3), kp_cur = pattern<double>(2 * m.nt, 4), b_ref = pattern<double>(3 * m.nt, 5), b_cur = pattern<double>(3 * m.nt, 6);
    std::vector<int32_t> oi(10 * m.np);
    std::vector<double> od(12 * m.np + 3 * m.nt);
    std::vector<float> of(8 * m.np);
    std::vector<uint8_t> ob(m.nt);
    F::Call c{m.handle, m.P, m.offsets, models.data(), mats.data(), cams.data(), inlier.data(), kp_ref.data(), kp_cur.data(), b_ref.data(), b_cur.data(),
              (float)getd(a, "reproj_err_thr", 4.0), (float)getd(a, "parallax_deg_thr", 1.0), oi.data(), oi.data() + m.np, od.data(), od.data() + 9 * m.np,
              oi.data() + 2 * m.np, of.data(), od.data() + 12 * m.np, ob.data()};
    NUL(models), NUL(mats), NUL(cams), NUL(inlier_flags), NUL(keypts_ref), NUL(keypts_cur), NUL(bearings_ref), NUL(bearings_cur), NUL(out_success),
        NUL(out_best), NUL(out_rot), NUL(out_trans), NUL(out_counts), NUL(out_parallax_deg), NUL(out_triangulated_pts), NUL(out_is_triangulated);
    if (g_bad) return false;
    const splan::Checked k = F::check(c, [&] { return splan::Caps{m.maxp, m.maxt, 0, 0}; });
    if (kind == "check") return print(k), true;
    if (!k.run) return false;
    const F::Layout lay = F::layout_of(m.P, k.T);
    Block b(lay.bytes);
    F::stage(c, lay, b.p);
    std::printf("%zu", lay.bytes), hex(b.p, b.bytes), std::printf("\n");
    return true;
}

bool run_triangulate(const std::string& kind, const Args& a) {
    namespace F = splan::triangulate;
    const Common m(a);
    const auto b1 = pattern<double>(3 * m.nt, 1), b2 = pattern<double>(3 * m.nt, 2);
    std::vector<std::vector<float>> f;
    f.push_back(pattern<float>(2 * m.nt, 3)), f.push_back(pattern<float>(2 * m.nt, 4));
    for (int id = 5; id < 13; ++id) f.push_back(pattern<float>(m.nt, id));
    const auto cams_1 = cameras(get(a, "cam1", "ok"), (int)m.np), cams_2 = cameras(get(a, "cam2", "equi"), (int)m.np);
    const auto poses_1 = pattern<double>(12 * m.np, 13), poses_2 = pattern<double>(12 * m.np, 14);
    std::vector<double> pos(3 * m.nt, -7.0);
    std::vector<uint8_t> status(m.nt, 9), method(m.nt, 9);
    std::vector<int32_t> num(m.np, -7);
    F::Call c{m.handle, m.P, m.offsets, b1.data(), b2.data(), f[0].data(), f[1].data(), f[2].data(), f[3].data(), f[4].data(), f[5].data(), f[6].data(),
              f[7].data(), f[8].data(), f[9].data(), cams_1.data(), cams_2.data(), poses_1.data(), poses_2.data(), getd(a, "cos_rays_parallax_thr", 0.9998),
              (float)getd(a, "ratio_factor", 1.8), pos.data(), status.data(), method.data(), num.data()};
    NUL(bearings_1), NUL(bearings_2), NUL(keypts_1), NUL(keypts_2), NUL(x_right_1), NUL(x_right_2), NUL(depths_1), NUL(depths_2), NUL(sigma_sq_1),
        NUL(sigma_sq_2), NUL(scale_factors_1), NUL(scale_factors_2), NUL(cams_1), NUL(cams_2), NUL(poses_cw_1), NUL(poses_cw_2), NUL(out_pos_w),
        NUL(out_status), NUL(out_method), NUL(out_num_accepted);
    if (g_bad) return false;
    const splan::Checked k = F::check(c, [&] { return splan::Caps{m.maxp, m.maxt, 0, 0}; });
    if (kind == "check") return print(k), true;
    if (!k.run) return false;
    const F::Layout lay = F::layout_of(m.P, k.T);
    Block b(lay.bytes);
    F::stage(c, lay, b.p);
    std::printf("%zu", lay.bytes), hex(b.p, b.bytes);
    double* out = reinterpret_cast<double*>(b.p + lay.pos);
    for (int32_t i = 0; i < 3 * k.T; ++i) out[i] = 1000.0 + i;
    for (int32_t i = 0; i < k.T; ++i) b.p[lay.status + (size_t)i] = (uint8_t)(i % 3);   // 0: accepted
    out_pattern(b.p + lay.method, (size_t)k.T, 2);
    F::collect(c, lay, b.p);
    hex(pos.data(), 24 * (size_t)k.T), hex(status.data(), (size_t)k.T), hex(method.data(), (size_t)k.T), hex(num.data(), 4 * (size_t)m.P);
    std::printf("\n");
    return true;
}

std::vector<splan::landmarks::KeyframeView> g_views;
splan::landmarks::KeyframeView view_of(const void* views, int32_t k) { return static_cast<const splan::landmarks::KeyframeView*>(views)[k]; }

// further keys: what, K, levels, res (1: the _f form), maxk, dev (the handle's device), kfdev (a device per keyframe, -1: a NULL entry), kfn (keypoints
// per keyframe), okf (obs_keyfrm; default t mod K), okp (obs_keypoint; default t), refk, refl (ref_keyfrm, ref_level; default 0 and p), use (obs_use; - NULL)
bool run_landmarks(const std::string& kind, const Args& a) {
    namespace F = splan::landmarks;
    const Common m(a);
    const int32_t K = geti(a, "K", 3), maxk = geti(a, "maxk", 6);
    const bool resident = geti(a, "res", 0) != 0;
    const int32_t dev = geti(a, "dev", 0);
    const size_t nk = (size_t)(K > maxk ? K : maxk > 0 ? maxk : 1);
    const auto fill = [&](const char* key, size_t n, auto dflt) {
        std::vector<int32_t> v = ints(get(a, key, ""));
        for (size_t i = v.size(); i < n; ++i) v.push_back(dflt(i));
        return v;
    };
    const auto okf = fill("okf", m.nt, [&](size_t t) { return K > 0 ? (int32_t)(t % (size_t)K) : 0; });
    const auto okp = fill("okp", m.nt, [](size_t t) { return (int32_t)t; });
    const auto refk = fill("refk", m.np, [](size_t) { return 0; });
    const auto refl = fill("refl", m.np, [](size_t p) { return (int32_t)p; });
    const auto kfdev = fill("kfdev", nk, [](size_t) { return 0; });
    const auto kfn = fill("kfn", nk, [](size_t) { return 100; });
    g_views.resize(nk);
    static uint8_t device_memory[64];   // addresses to stand for the keyframes' descriptors; never read
    for (size_t i = 0; i < nk; ++i) g_views[i] = F::KeyframeView{kfdev[i], kfn[i], kfdev[i] < 0 ? nullptr : device_memory + (i % 64)};
    std::vector<uint8_t> use;
    const std::string use_text = get(a, "use", "-");
    if (use_text != "-")
        for (const int32_t u : ints(use_text)) use.push_back((uint8_t)u);
    if (use_text != "-" && use.size() != (size_t)m.T) g_bad = true;
    const auto pos_w = pattern<double>(3 * m.np, 1);
    const auto desc = pattern<uint8_t>(32 * m.nt, 2);
    const auto centres = pattern<double>(3 * nk, 3);
    const auto sf = pattern<float>(OVS_MAX_LEVELS, 4);
    std::vector<double> normal(3 * m.np, -7.0);
    std::vector<float> range(2 * m.np, -7.0f);
    std::vector<int32_t> best(m.np, -7);
    std::vector<uint8_t> out_desc(32 * m.np, 9), status(m.np, 9);
    F::Call c{m.handle, geti(a, "what", 3), m.P, m.offsets, pos_w.data(), refk.data(), refl.data(), okf.data(), resident ? nullptr : desc.data(), resident,
              resident ? g_views.data() : nullptr, resident ? view_of : nullptr, resident ? okp.data() : nullptr, use_text == "-" ? nullptr : use.data(),
              centres.data(), K, sf.data(), geti(a, "levels", 8), normal.data(), range.data(), best.data(), out_desc.data(), status.data()};
    NUL(pos_w), NUL(ref_keyfrm), NUL(ref_level), NUL(obs_keyfrm), NUL(obs_desc), NUL(keyfrms), NUL(obs_keypoint), NUL(cam_centers), NUL(scale_factors),
        NUL(out_mean_normal), NUL(out_min_max_dist), NUL(out_best_obs), NUL(out_desc), NUL(out_status);
    if (g_bad) return false;
    const splan::Checked k = F::check(c, [&] { return splan::Caps{m.maxp, m.maxt, maxk, dev}; });
    if (kind == "check") return print(k), true;
    if (!k.run) return false;
    const F::Layout lay = F::layout_for(c, k.T);
    Block b(lay.total), table(F::table_bytes(maxk));
    const F::Lists lists = F::stage(c, lay, b.p, table.p);
    std::printf("%zu %zu", lay.bytes, lay.total), hex(b.p, b.bytes), std::printf(" %d %d", (int)lists.n8, (int)lists.n64);
    if (resident)   // the pointers as the keyframe's number + 1 (0: NULL)
        for (int32_t i = 0; i < K; ++i) {
            const uint8_t* p;
            std::memcpy(&p, table.p + F::table_ptrs_at(K) + 8 * (size_t)i, 8);
            std::memset(table.p + F::table_ptrs_at(K) + 8 * (size_t)i, p ? (int)(p - device_memory) + 1 : 0, 8);
        }
    hex(table.p, table.bytes);
    double* nrm = reinterpret_cast<double*>(b.p + lay.normal);
    float* rng = reinterpret_cast<float*>(b.p + lay.range);
    int32_t* bst = reinterpret_cast<int32_t*>(b.p + lay.best);
    for (int32_t i = 0; i < 3 * m.P; ++i) nrm[i] = 1000.0 + i;
    for (int32_t i = 0; i < 2 * m.P; ++i) rng[i] = 2000.0f + (float)i;
    for (int32_t p = 0; p < m.P; ++p) bst[p] = m.offsets[p] + 1;
    out_pattern(b.p + lay.out_desc, 32 * (size_t)m.P, 3);
    F::collect(c, lay, b.p);
    hex(normal.data(), 24 * (size_t)m.P), hex(range.data(), 8 * (size_t)m.P), hex(best.data(), 4 * (size_t)m.P), hex(out_desc.data(), 32 * (size_t)m.P),
        hex(status.data(), (size_t)m.P);
    std::printf("\n");
    return true;
}

template <class L>
void print_layout(const L& l) {   // a Layout is size_t members only
    size_t v[sizeof(L) / sizeof(size_t)];
    std::memcpy(v, &l, sizeof(L));
    for (size_t i = 0; i < sizeof(L) / sizeof(size_t); ++i) std::printf(i ? " %zu" : "%zu", v[i]);
    std::printf("\n");
}

bool layout(const std::string& fam, const Args& a) {
    const int P = geti(a, "P", 1), T = geti(a, "T", 0);
    if (g_bad || P < 1 || T < 0) return false;
    if (fam == "sim3") print_layout(splan::sim3::layout_of(P, T));
    else if (fam == "pnp") print_layout(splan::pnp::layout_of(P, T));
    else if (fam == "sim3opt") print_layout(splan::sim3opt::layout_of(P, T));
    else if (fam == "twoview") print_layout(splan::twoview::layout_of(P, T));
    else if (fam == "essential") print_layout(splan::essential::layout_of(P, T));
    else if (fam == "reconstruct") print_layout(splan::reconstruct::layout_of(P, T));
    else if (fam == "triangulate") print_layout(splan::triangulate::layout_of(P, T));
    else if (fam == "landmarks" && geti(a, "desc", 0)) print_layout(splan::landmarks::layout_of<true>(P, T));
    else if (fam == "landmarks") print_layout(splan::landmarks::layout_of<false>(P, T));
    else return false;
    return true;
}

bool row(const std::string& text) {
    const std::vector<std::string> v = split(text, ':');
    if (v.size() < 2) return false;
    Args a;
    for (size_t i = 2; i < v.size(); ++i) {
        const size_t eq = v[i].find('=');
        if (eq == std::string::npos) return false;
        a[v[i].substr(0, eq)] = v[i].substr(eq + 1);
    }
    g_bad = false;
    const std::string &kind = v[0], &fam = v[1];
    if (kind == "layout") return layout(fam, a);
    if (kind != "check" && kind != "stage") return false;
    if (fam == "sim3") return run_sim3(kind, a);
    if (fam == "pnp") return run_pnp(kind, a);
    if (fam == "sim3opt") return run_sim3opt(kind, a);
    if (fam == "twoview") return run_twoview(kind, a);
    if (fam == "essential") return run_essential(kind, a);
    if (fam == "reconstruct") return run_reconstruct(kind, a);
    if (fam == "triangulate") return run_triangulate(kind, a);
    if (fam == "landmarks") return run_landmarks(kind, a);
    return false;
}

}   // namespace

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        if (!row(line)) {
            std::fprintf(stderr, "bad row: %s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
