// ba_optimize.hip -- B4: optimize::local_bundle_adjuster::optimize, the part behind the graph build (expected:
// src/openvslam/optimize/local_bundle_adjuster.cc; g2o OptimizationAlgorithmLevenberg + BlockSolver_6_3 with Schur complement).
//
// The caller (the class shim) flattens the local map into poses / landmarks / observation edges; this file runs what
// optimizer.optimize(num_first_iter) -> outlier levels -> optimizer.optimize(num_second_iter) does, on top of ba_graph.hip:
//   * the state (poses as SE3Quat records, points) and both block sets (current system / trial system) live in HBM for the whole call;
//   * one Levenberg-Marquardt trial = six launches on the device (round 6: k_lm_prepare, k_schur_l, the dense solver of ba_solve.hip,
//     k_trial_update, k_linearize2, k_reduce_scalars: ~230 us at config 5) whose outcome the host polls from twelve flag-carrying words in
//     page-locked memory (OVS_BA_LL_NOTIFY=0: ONE 260-byte download); with ovs_local_ba_set_solver(1) (BASELINE's north star keeps the
//     Cholesky of the reduced camera system on the HOST; at most 6 n_pose square) a 0.7 MB download (S | rhs | bp), 2.4 KB of pose increments
//     up, k_backsub, the SE3 update of <= 50 poses on the host, and the linearisation of the trial state;
//   * g2o's damping schedule (ORACLE_SPEC rule 25), the chi-square outlier gates between the two rounds and the final outlier flags.
// Round 1: 16 MB per trial crossed PCIe and the landmark elimination ran on 8 host threads (117 ms at config 5).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ba_host_math.h"
#include "ba_internal.h"
#include "ba_pcg_internal.inc"
#include "owned_internal.inc"

namespace ovs {
std::atomic<int> g_lba_solver{0};
}   // namespace ovs

namespace {

using namespace ovs_ba_host;
using ovs::ArenaLayout;
using ovs::set_last_error;

// upstream: constexpr float chi_sq_2D = 5.99146, chi_sq_3D = 7.81473 and their float square roots, widened to double where g2o consumes them
constexpr double kChi2D = 0x1.7f7414p+2, kChi3D = 0x1.f4248ap+2, kSqrtChi2D = 0x1.394fbcp+1, kSqrtChi3D = 0x1.65d26ap+1;

struct DevBlocks {   // one linearisation in HBM: Hpp | bp | Hll | bl | Hpl | chi2[2], max|diag|
    double *Hpp = nullptr, *bp = nullptr, *Hll = nullptr, *bl = nullptr, *Hpl = nullptr, *chi = nullptr;
    static size_t doubles(int n_pose, int n_pt, size_t n_edge) { return (size_t)42 * n_pose + (size_t)12 * n_pt + 18 * std::max<size_t>(n_edge, 1) + 4; }
    void carve(double* base, int n_pose, int n_pt, size_t n_edge) {
        Hpp = base;
        bp = Hpp + (size_t)36 * n_pose;
        Hll = bp + (size_t)6 * n_pose;
        bl = Hll + (size_t)9 * n_pt;
        Hpl = bl + (size_t)3 * n_pt;
        chi = Hpl + 18 * std::max<size_t>(n_edge, 1);
    }
};

// A trial's outcome on the host. It sits in page-locked memory behind the system and the staging area (pin_layout): the copies and the last
// kernel of a trial write it, the host reads it.
struct TrialBlock {   // image of the solver arena's d_scal | d_fail: the ONE download per trial of OVS_BA_LL_NOTIFY=0
    double scal[32];   // [0] landmarks' / [1] keyframes' part of the gain ratio's denominator, [2..4] the trial state's chi2 triple
    int32_t fail[2];
};
static_assert(sizeof(TrialBlock) == 256 + 2 * sizeof(int32_t), "d_fail sits 256 bytes behind d_scal");
struct Mailbox {
    double chi[3];               // chi2, robustified chi2, the largest |diagonal entry| of the linearisation last read
    double scale_lm, scale_kf;   // the gain ratio's denominator: the landmarks' and the keyframes' part
    int32_t fail;                // the trial's failure word
    TrialBlock blk;
    ovs::PcgHostBlock pcg;       // what a conjugate-gradient solve brings down (global BA)
    volatile unsigned long long ll[16];   // k_reduce_scalars' flag-carrying words {seq : 32 | half a double : 32}, twelve in use
};
struct PinLayout {
    size_t stage, mailbox, bytes;   // (the padded system | bp come first, at offset 0)
};
// `host_system`: room for the system as the host solver downloads it (global BA never takes that path: 300 MB at 1024 keyframes)
static PinLayout pin_layout(int n_pose, bool host_system) {
    ArenaLayout lay;
    PinLayout p;
    lay.place<double>(host_system ? ovs::dense_solve_doubles(6 * n_pose) + 6 * (size_t)n_pose : 0);
    p.stage = lay.place<double>(19 * (size_t)n_pose);   // the keyframes' records on their way up: 7 + 12 per keyframe
    p.mailbox = lay.place<Mailbox>(1);
    p.bytes = lay.bytes();
    return p;
}

// Per-thread work space that only grows: local BA runs once per keyframe on the mapping thread, and a dozen hipMalloc / hipHostMalloc /
// stream-create calls per call (3-5 ms) would cost as much as the optimisation itself.
struct LmScratch {
    int device = -1;
    hipStream_t stream = nullptr;
    unsigned char* d = nullptr;
    size_t d_cap = 0;
    ovs::PinnedBuffer pin;    // pin_layout
    ovs::PinnedBuffer edge;   // round 1's inlier count (4 bytes), then the final outlier flags (one byte per edge)
    ovs::PinnedBuffer pts;    // the landmarks on their way up (start of the call) and down (its end)
    ovs::Owned res;           // d and stream
    void release() {          // (the work space moves to another device)
        (void)res.drop(&d);
        d_cap = 0;
        pin.release();
        edge.release();
        pts.release();
        (void)res.drop(&stream);
    }
};

struct Trial {   // what one Levenberg-Marquardt trial tells the damping schedule
    bool ok = false;
    double temp_chi = 1.7976931348623157e308, scale = 1e-3;
};

struct Lm {
    int n_pose = 0, n_pt = 0, setup_type = 0;
    // OVS_BA_TRACE=1: wall-clock breakdown on stderr (where a call's milliseconds go; tools/time_lba.py)
    double t_schur = 0, t_chol = 0, t_trial = 0;
    int n_trials = 0;
    // global BA: the deltas come from the caller (0.0 = no kernel) instead of the rig; what the conjugate-gradient solves and the trials did
    bool huber_given = false;
    double huber_mono_given = 0.0, huber_stereo_given = 0.0;
    long long pcg_iterations = 0;
    int pcg_capped = 0, failed_solves = 0, n_accepted = 0;
    bool err_at_trial = false;   // the active edges' errors were last computed at the trial state (d_poses_n, d_Xn), which was then rejected
    static double now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    hipStream_t stream = nullptr;
    DevBlocks cur, trial, work;   // accepted state | last evaluated trial | where the next trial is evaluated (device solver only)
    double *d_poses = nullptr, *d_poses_n = nullptr, *d_poses_w = nullptr, *d_X = nullptr, *d_Xn = nullptr, *d_Xw = nullptr, *d_echi = nullptr;
    double *d_T = nullptr, *d_Tn = nullptr, *d_Tw = nullptr;   // R | t per keyframe (12 doubles), the state k_pose_update advances
    uint8_t* d_edepth = nullptr;
    // the outlier gates on the device (round 6): round 1's chi2 per edge (kept for the final verdict of level-1 edges), a second chi2 array for the
    // launch whose chi2 nobody reads, round 1's and the final flags, the inlier count
    double *d_echi_r1 = nullptr, *d_echi_s = nullptr;
    uint8_t *d_out1 = nullptr, *d_outf = nullptr;
    int32_t* d_nact = nullptr;
    double* h_pts = nullptr;     // LmScratch::pts
    double* h_sys = nullptr;     // LmScratch::pin: S | rhs | bp as the host solver downloads them
    double* h_stage = nullptr;   //                 the keyframes' records on their way up
    Mailbox* mb = nullptr;       //                 a trial's outcome
    unsigned char* h_edge = nullptr;   // LmScratch::edge
    bool ll_notify = true;

    ovs_status init(int device, int np, int npt, size_t ne_max, const double* points, bool host_system = true) {
        static thread_local LmScratch sc;
        n_pose = np;
        n_pt = npt;
        if (sc.device != device) {
            sc.release();
            sc.device = device;
        }
        if (!sc.stream) OVS_HIP_TRY(sc.res.stream(&sc.stream));
        stream = sc.stream;
        const size_t ne = std::max<size_t>(ne_max, 1), nd = DevBlocks::doubles(np, npt, ne_max);
        ArenaLayout lay;
        const size_t o_cur = lay.place<double>(nd), o_trial = lay.place<double>(nd), o_work = lay.place<double>(nd);
        const size_t o_p = lay.place<double>(7 * (size_t)np), o_pn = lay.place<double>(7 * (size_t)np), o_pw = lay.place<double>(7 * (size_t)np);
        const size_t o_x = lay.place<double>(3 * (size_t)npt), o_xn = lay.place<double>(3 * (size_t)npt), o_xw = lay.place<double>(3 * (size_t)npt);
        const size_t o_t = lay.place<double>(12 * (size_t)np), o_tn = lay.place<double>(12 * (size_t)np), o_tw = lay.place<double>(12 * (size_t)np);
        const size_t o_echi = lay.place<double>(ne), o_edepth = lay.place<uint8_t>(ne), o_echi_r1 = lay.place<double>(ne), o_echi_s = lay.place<double>(ne);
        const size_t o_out1 = lay.place<uint8_t>(ne), o_outf = lay.place<uint8_t>(ne), o_nact = lay.place<int32_t>(1);
        if (sc.d_cap < lay.bytes()) {
            (void)sc.res.drop(&sc.d);
            sc.d_cap = 0;
            OVS_HIP_TRY(sc.res.dev(&sc.d, lay.bytes()));
            sc.d_cap = lay.bytes();
        }
        cur.carve(ArenaLayout::at<double>(sc.d, o_cur), np, npt, ne_max);
        trial.carve(ArenaLayout::at<double>(sc.d, o_trial), np, npt, ne_max);
        work.carve(ArenaLayout::at<double>(sc.d, o_work), np, npt, ne_max);
        d_poses = ArenaLayout::at<double>(sc.d, o_p), d_poses_n = ArenaLayout::at<double>(sc.d, o_pn), d_poses_w = ArenaLayout::at<double>(sc.d, o_pw);
        d_X = ArenaLayout::at<double>(sc.d, o_x), d_Xn = ArenaLayout::at<double>(sc.d, o_xn), d_Xw = ArenaLayout::at<double>(sc.d, o_xw);
        d_T = ArenaLayout::at<double>(sc.d, o_t), d_Tn = ArenaLayout::at<double>(sc.d, o_tn), d_Tw = ArenaLayout::at<double>(sc.d, o_tw);
        d_echi = ArenaLayout::at<double>(sc.d, o_echi), d_echi_r1 = ArenaLayout::at<double>(sc.d, o_echi_r1), d_echi_s = ArenaLayout::at<double>(sc.d, o_echi_s);
        d_edepth = sc.d + o_edepth, d_out1 = sc.d + o_out1, d_outf = sc.d + o_outf;
        d_nact = ArenaLayout::at<int32_t>(sc.d, o_nact);
        const PinLayout pl = pin_layout(np, host_system);
        OVS_HIP_TRY(sc.pin.ensure(pl.bytes, pl.bytes));
        h_sys = ArenaLayout::at<double>(sc.pin.p, 0);
        h_stage = ArenaLayout::at<double>(sc.pin.p, pl.stage);
        mb = ArenaLayout::at<Mailbox>(sc.pin.p, pl.mailbox);
        // (pageable std::vectors here cost a staged 0.9 MB copy and fresh pages twice per call: ~0.3 ms of a 7.7 ms call)
        OVS_HIP_TRY(sc.edge.ensure(ne, (ne + 1023) & ~(size_t)1023));
        h_edge = sc.edge.p;
        const size_t n3 = (size_t)3 * npt;
        OVS_HIP_TRY(sc.pts.ensure(sizeof(double) * n3, sizeof(double) * ((n3 + n3 / 4 + 511) & ~(size_t)511)));
        h_pts = reinterpret_cast<double*>(sc.pts.p);
        // through the page-locked block, no wait: the landmarks travel while the caller (ovs_local_ba_optimize) indexes the edges; the block is
        // written next at the end of the call, behind a dozen stream synchronisations
        std::memcpy(h_pts, points, sizeof(double) * n3);
        OVS_HIP_TRY(hipMemcpyAsync(d_X, h_pts, sizeof(double) * n3, hipMemcpyHostToDevice, stream));
        return OVS_OK;
    }

    static void pack_poses(const std::vector<Pose>& T, std::vector<double>& p7) {
        p7.resize(7 * T.size());
        for (size_t k = 0; k < T.size(); ++k) {
            p7[7 * k] = T[k].t[0];
            p7[7 * k + 1] = T[k].t[1];
            p7[7 * k + 2] = T[k].t[2];
            rot_to_quat(T[k].R, &p7[7 * k + 3]);
        }
    }

    // the 7-double records (and, for the device solver, R | t) of all keyframes through the page-locked staging area: no wait here -- the area is
    // written again only at the start of the next round, long after the round's first stream synchronisation
    ovs_status upload_poses(const std::vector<Pose>& T, double* dst, double* dst_rt) {
        std::vector<double> p7;
        pack_poses(T, p7);
        double* const st7 = h_stage;
        std::memcpy(st7, p7.data(), sizeof(double) * p7.size());
        OVS_HIP_TRY(hipMemcpyAsync(dst, st7, sizeof(double) * p7.size(), hipMemcpyHostToDevice, stream));
        if (dst_rt) {
            double* const rt = st7 + 7 * (size_t)n_pose;
            for (int k = 0; k < n_pose; ++k) {
                std::memcpy(rt + (size_t)12 * k, T[k].R, sizeof(double) * 9);
                std::memcpy(rt + (size_t)12 * k + 9, T[k].t, sizeof(double) * 3);
            }
            OVS_HIP_TRY(hipMemcpyAsync(dst_rt, rt, sizeof(double) * 12 * (size_t)n_pose, hipMemcpyHostToDevice, stream));
        }
        return OVS_OK;
    }

    double huber_mono(bool robust) const { return !robust ? 0.0 : huber_given ? huber_mono_given : setup_type == 0 ? kSqrtChi2D : kSqrtChi3D; }
    double huber_stereo(bool robust) const { return !robust ? 0.0 : huber_given ? huber_stereo_given : kSqrtChi3D; }

    // Round 6: the trial's last kernel wrote the outcome into the mailbox as twelve words {seq | half a double}; poll them (no copy command, no
    // stream wait). Every 4096 polls the stream is asked whether it still runs: a launch that died would otherwise never write the words.
    // False: the stream went idle (or failed) without the words -- the copy path decides.
    bool poll_flag_words(unsigned int seq, unsigned long long (&w)[12]) {
        unsigned int spins = 0;
        for (int i = 0; i < 12;) {
            w[i] = mb->ll[i];
            if ((unsigned int)(w[i] >> 32) == seq) {
                ++i;
                continue;
            }
            if ((++spins & 4095u) == 0u && hipStreamQuery(stream) != hipErrorNotReady) {   // idle (or failed): one last look
                w[i] = mb->ll[i];
                if ((unsigned int)(w[i] >> 32) != seq) return false;
            }
        }
        return true;
    }

    // ---- one trial, the whole of it on the device: Schur complement, solve, keyframe / landmark updates, linearisation at the trial state (into
    //      the `work` set: a failed solve must leave the last evaluated trial state, which edge_chi2 may still need, untouched)
    //      `solver`: 1 = ba_solve.hip's Cholesky, 2 = ba_pcg.hip's conjugate gradient (global BA beyond the Cholesky's size), which reads S only
    ovs_status trial_on_device(ovs_ba_graph* g, const ovs::BaGraphInfo& gi, int n, double lambda, bool robust, Trial& r, int solver = 1) {
        const double t0 = now();
        const int fw = n_trials & 1;   // the trials alternate between two failure words
        ovs_status st = ovs::ba_graph_schur(g, cur.Hpp, cur.bp, cur.Hll, cur.bl, cur.Hpl, lambda, stream, fw, false);
        if (st != OVS_OK) return st;
        if (n > 0 && solver == 2) {
            unsigned char* d_pcg = nullptr;
            st = ovs::ba_graph_pcg_arena(g, &d_pcg);
            if (st != OVS_OK) return st;
            ovs::PcgResult pr;
            st = ovs::launch_pcg_solve(gi.d_S, gi.s_pitch, gi.d_rhs, n, gi.d_fail + fw, d_pcg, &mb->pcg, 1e-10, 0, 0, stream, &pr);
            if (st != OVS_OK) return st;
            pcg_iterations += pr.iterations;
            pcg_capped += pr.capped ? 1 : 0;
        } else if (n > 0) {
            st = ovs::launch_dense_solve(gi.d_S, n, gi.d_fail + fw, stream);
            if (st != OVS_OK) return st;
        }
        st = ovs::ba_graph_trial_update(g, d_T, cur.bp, cur.Hpl, cur.bl, lambda, d_Tw, d_poses_w, d_X, d_Xw, stream, fw ^ 1);
        if (st != OVS_OK) return st;
        // the trial state's chi2 triple is mirrored next to the solver's scalars (gi.d_scal[2..4]; gi.d_fail sits 256 bytes behind gi.d_scal in
        // the same arena): ONE 264-byte download per trial instead of three copies (round 5: two copy launches and their gaps less per trial).
        // (One kernel writing the values straight into the page-locked block was measured in round 4 -- the system-scope flush at its end costs
        // ~50 us per trial.)
        static thread_local unsigned int ll_seq = 0;   // sequence number of a trial's words: per thread, like the page-locked block they land in
        const unsigned int seq = ++ll_seq == 0u ? ++ll_seq : ll_seq;   // (never 0: the block starts zeroed)
        st = ovs::ba_graph_linearize(g, d_poses_w, d_Xw, huber_mono(robust), huber_stereo(robust), work.Hpp, work.bp, work.Hll, work.bl, work.Hpl,
                                     work.chi, stream, gi.d_scal + 2, true, ll_notify ? const_cast<unsigned long long*>(mb->ll) : nullptr, seq);
        if (st != OVS_OK) return st;
        unsigned long long w[12];
        if (ll_notify && poll_flag_words(seq, w)) {
            auto val = [&](int i) {
                const unsigned long long bits = (w[2 * i] & 0xffffffffull) | (w[2 * i + 1] << 32);
                double d;
                std::memcpy(&d, &bits, sizeof(d));
                return d;
            };
            mb->scale_lm = val(0);
            mb->scale_kf = val(1);
            mb->chi[0] = val(2);
            mb->chi[1] = val(3);
            mb->chi[2] = val(4);   // (the largest |diagonal| of the LANDMARKS only, not the full maximum of the start damping: nothing reads it after a trial)
            mb->fail = (int32_t)(uint32_t)(w[10 + fw] & 0xffffffffull);
        } else {
            OVS_HIP_TRY(hipMemcpyAsync(&mb->blk, gi.d_scal, sizeof(TrialBlock), hipMemcpyDeviceToHost, stream));
            OVS_HIP_TRY(hipStreamSynchronize(stream));   // (polling hipStreamQuery instead: the same 6.5-6.6 ms per call, round 5)
            mb->scale_lm = mb->blk.scal[0];
            mb->scale_kf = mb->blk.scal[1];
            mb->chi[0] = mb->blk.scal[2];
            mb->chi[1] = mb->blk.scal[3];
            mb->chi[2] = mb->blk.scal[4];   // (the landmarks' largest |diagonal| only, as in the flag words)
            mb->fail = mb->blk.fail[fw];
        }
        r.ok = mb->fail == 0;
        failed_solves += r.ok ? 0 : 1;
        if (!r.ok) {   // a failed factorisation may have left non-finite values in the padding, which no later trial rewrites
            st = ovs::ba_graph_reset_system(g, stream);
            if (st != OVS_OK) return st;
        } else {
            r.temp_chi = mb->chi[1];
            r.scale = (mb->scale_kf + mb->scale_lm) + 1e-3;   // keyframes' part, then the landmarks' (g2o's computeScale order)
            std::swap(trial, work);
            std::swap(d_poses_n, d_poses_w);
            std::swap(d_Xn, d_Xw);
            std::swap(d_Tn, d_Tw);
            err_at_trial = true;
        }
        t_trial += now() - t0;
        return OVS_OK;
    }
    void accept_on_device() {
        ++n_accepted;
        std::swap(d_X, d_Xn);
        std::swap(d_poses, d_poses_n);
        std::swap(d_T, d_Tn);
        std::swap(cur, trial);
    }

    // ---- one trial with the reduced camera system solved on the host: 0.7 MB (S | rhs | bp) down, the keyframes' increments and records up,
    //      k_backsub, the linearisation of the trial state
    struct HostState {
        std::vector<Pose>& T;   // the accepted keyframes
        std::vector<Pose> Tn;   // the trial's
        std::vector<double> S, rhs, dxp;
    };
    ovs_status trial_on_host(ovs_ba_graph* g, const ovs::BaGraphInfo& gi, int n, double lambda, bool robust, HostState& h, Trial& r) {
        const double t0 = now();
        ovs_status st = ovs::ba_graph_schur(g, cur.Hpp, cur.bp, cur.Hll, cur.bl, cur.Hpl, lambda, stream, 0, true);
        if (st != OVS_OK) return st;
        const size_t np_ = (size_t)gi.s_pitch, sys_rows = np_ + 1;   // S rows and the rhs row
        const double* const h_bp = h_sys + sys_rows * np_;
        if (n > 0) {
            OVS_HIP_TRY(hipMemcpyAsync(h_sys, gi.d_S, sizeof(double) * sys_rows * np_, hipMemcpyDeviceToHost, stream));
            OVS_HIP_TRY(hipMemcpyAsync(h_sys + sys_rows * np_, cur.bp, sizeof(double) * 6 * (size_t)n_pose, hipMemcpyDeviceToHost, stream));
        }
        OVS_HIP_TRY(hipMemcpyAsync(&mb->fail, gi.d_fail, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
        OVS_HIP_TRY(hipStreamSynchronize(stream));
        r.ok = mb->fail == 0;
        const double t1 = now();
        t_schur += t1 - t0;
        if (r.ok && n > 0) {
            h.S.resize((size_t)n * n);
            for (int i = 0; i < n; ++i) std::memcpy(&h.S[(size_t)i * n], h_sys + (size_t)i * np_, sizeof(double) * n);   // drop the padding
            h.rhs.assign(h_sys + np_ * np_, h_sys + np_ * np_ + n);
            r.ok = cholesky_solve(h.S, n, h.rhs);
        }
        const double t2 = now();
        t_chol += t2 - t1;
        if (r.ok) {
            std::vector<double>& dxp = h.dxp;
            dxp.assign((size_t)6 * n_pose, 0.0);
            h.Tn = h.T;
            for (int k = 0; k < n_pose; ++k)
                if (gi.slot[k] >= 0) {
                    for (int a = 0; a < 6; ++a) dxp[(size_t)6 * k + a] = h.rhs[(size_t)6 * gi.slot[k] + a];
                    se3_oplus(h.Tn[k], &dxp[(size_t)6 * k]);
                }
            std::vector<double> p7;
            pack_poses(h.Tn, p7);
            OVS_HIP_TRY(hipMemcpyAsync(gi.d_dxp, dxp.data(), sizeof(double) * dxp.size(), hipMemcpyHostToDevice, stream));
            OVS_HIP_TRY(hipMemcpyAsync(d_poses_n, p7.data(), sizeof(double) * p7.size(), hipMemcpyHostToDevice, stream));
            st = ovs::ba_graph_backsub(g, cur.Hpl, cur.bl, lambda, d_X, d_Xn, stream);
            if (st != OVS_OK) return st;
            st = ovs::ba_graph_linearize(g, d_poses_n, d_Xn, huber_mono(robust), huber_stereo(robust), trial.Hpp, trial.bp, trial.Hll, trial.bl,
                                         trial.Hpl, trial.chi, stream, nullptr, true);
            if (st != OVS_OK) return st;
            OVS_HIP_TRY(hipMemcpyAsync(mb->chi, trial.chi, sizeof(double) * 3, hipMemcpyDeviceToHost, stream));
            OVS_HIP_TRY(hipMemcpyAsync(&mb->scale_lm, gi.d_scal, sizeof(double), hipMemcpyDeviceToHost, stream));
            OVS_HIP_TRY(hipStreamSynchronize(stream));   // also covers dxp / p7 (locals)
            r.temp_chi = mb->chi[1];
            err_at_trial = true;   // computeActiveErrors() ran on the trial state (d_poses_n, d_Xn); cleared when it is accepted
            double sc = 0;
            for (int k = 0; k < n_pose; ++k)
                if (gi.slot[k] >= 0)
                    for (int a = 0; a < 6; ++a) sc += dxp[(size_t)6 * k + a] * (lambda * dxp[(size_t)6 * k + a] + h_bp[(size_t)6 * k + a]);
            r.scale = (sc + mb->scale_lm) + 1e-3;
        }
        t_trial += now() - t2;
        return OVS_OK;
    }
    void accept_on_host(HostState& h) {
        h.T.swap(h.Tn);
        std::swap(d_X, d_Xn);
        std::swap(d_poses, d_poses_n);
        std::swap(cur, trial);   // the accepted trial's blocks are the next iteration's system
    }

    // g2o's OptimizationAlgorithmLevenberg::solve around `trial` (one trial at damping lambda) and `accept` (the trial state becomes the
    // estimate): the damping schedule of ORACLE_SPEC rule 25
    template <class TrialFn, class AcceptFn>
    ovs_status lm_iterate(TrialFn trial_fn, AcceptFn accept, int iters, const volatile uint8_t* stop, double lambda, double* current_chi, int* n_iter) {
        double ni = 2;
        for (int it = 0; it < iters; ++it) {
            if (stop && *stop) break;
            ++*n_iter;
            double rho = 0;
            int qmax = 0;
            err_at_trial = false;   // solve() starts with computeActiveErrors() at the current estimate
            do {
                ++n_trials;
                Trial r;
                const ovs_status st = trial_fn(lambda, r);
                if (st != OVS_OK) return st;
                rho = (*current_chi - r.temp_chi) / r.scale;
                if (r.ok && rho > 0 && std::isfinite(r.temp_chi)) {
                    double alpha = 1.0 - std::pow(2 * rho - 1, 3.0);
                    alpha = std::min(alpha, 2.0 / 3.0);
                    lambda *= std::max(1.0 / 3.0, alpha);
                    ni = 2;
                    *current_chi = r.temp_chi;
                    accept();
                    err_at_trial = false;   // the trial state is the estimate now
                } else {
                    lambda *= ni;
                    ni *= 2;
                    if (!std::isfinite(lambda)) break;
                }
                ++qmax;
            } while (rho < 0 && qmax < 10 && !(stop && *stop));
            if (qmax == 10 || rho == 0 || !std::isfinite(lambda)) break;
        }
        return OVS_OK;
    }

    // one optimizer.optimize(iters) call on graph g. Returns the number of iterations entered.
    // `solver`: 0 = local BA's selection (below), 1 / 2 = trial_on_device's (global BA, which has chosen by size)
    ovs_status run_round(ovs_ba_graph* g, std::vector<Pose>& T, int iters, bool robust, const volatile uint8_t* stop, double* chi_start,
                         double* chi_end, int* n_iter, int solver = 0) {
        ovs_status st = ovs::ba_graph_ensure_solver(g, stream);   // (before ba_graph_info: the work space is allocated on first use)
        if (st != OVS_OK) return st;
        const ovs::BaGraphInfo gi = ovs::ba_graph_info(g);
        const int n = 6 * gi.n_free;
        // the reduced camera system is solved where ovs_local_ba_set_solver says; systems beyond the one-workgroup solver's LDS go to the host
        const bool dev_solve = solver != 0 || (ovs::g_lba_solver.load(std::memory_order_relaxed) == 0 && n <= ovs::dense_solve_max_n());
        st = upload_poses(T, d_poses, dev_solve ? d_T : nullptr);
        if (st != OVS_OK) return st;
        // both failure words start a round clear: the device solver's trials rely on the PREVIOUS trial's k_trial_update to clear the word they
        // are about to use, which a round that ran on the host solver (ovs_local_ba_set_solver between rounds) has not done
        if (dev_solve) OVS_HIP_TRY(hipMemsetAsync(gi.d_fail, 0, 2 * sizeof(int32_t), stream));
        st = ovs::ba_graph_linearize(g, d_poses, d_X, huber_mono(robust), huber_stereo(robust), cur.Hpp, cur.bp, cur.Hll, cur.bl, cur.Hpl, cur.chi,
                                     stream);
        if (st != OVS_OK) return st;
        for (int i = 0; i < 16; ++i) mb->ll[i] = 0ull;   // (the stream is idle here; whatever the block's last user left cannot pass for a word)
        ll_notify = ovs::tuning().ba_ll_notify;   // OVS_BA_LL_NOTIFY=0: a trial's outcome through a D2H copy and a stream synchronisation (rounds 4-5)
        OVS_HIP_TRY(hipMemcpyAsync(mb->chi, cur.chi, sizeof(double) * 3, hipMemcpyDeviceToHost, stream));
        OVS_HIP_TRY(hipStreamSynchronize(stream));
        double current_chi = mb->chi[1];
        *chi_start = current_chi;
        *chi_end = current_chi;
        *n_iter = 0;
        err_at_trial = false;
        if (iters <= 0) return OVS_OK;
        const double lambda0 = 1e-5 * mb->chi[2];   // computeLambdaInit: tau * the largest diagonal entry of the active vertices' Hessian blocks
        if (dev_solve) {
            st = lm_iterate([&](double lambda, Trial& r) { return trial_on_device(g, gi, n, lambda, robust, r, solver == 2 ? 2 : 1); },
                            [&] { accept_on_device(); }, iters, stop, lambda0, &current_chi, n_iter);
        } else {
            HostState h{T, {}, {}, {}, {}};
            st = lm_iterate([&](double lambda, Trial& r) { return trial_on_host(g, gi, n, lambda, robust, h, r); }, [&] { accept_on_host(h); }, iters,
                            stop, lambda0, &current_chi, n_iter);
        }
        if (st != OVS_OK) return st;
        *chi_end = current_chi;
        if (dev_solve) {   // the accepted keyframe state comes back once per round
            std::vector<double> rt((size_t)12 * n_pose);
            OVS_HIP_TRY(hipMemcpyAsync(rt.data(), d_T, sizeof(double) * rt.size(), hipMemcpyDeviceToHost, stream));
            OVS_HIP_TRY(hipStreamSynchronize(stream));
            for (int k = 0; k < n_pose; ++k) {
                std::memcpy(T[k].R, &rt[(size_t)12 * k], sizeof(double) * 9);
                std::memcpy(T[k].t, &rt[(size_t)12 * k + 9], sizeof(double) * 3);
            }
        }
        return OVS_OK;
    }

    // What upstream reads after optimizer.optimize(): edge->chi2() -- the error STORED by the last computeActiveErrors(), i.e. at the last
    // LM trial state when the round ended on a rejected step (g2o pops the estimate back but leaves the errors) -- and
    // edge->depth_is_positive(), which is evaluated from the vertices' current, accepted estimates (T, d_X). Evaluated on the device (round 6):
    // the chi2 upstream would read goes to `d_chi_judged`, the depth flags of the accepted state to d_edepth. Nothing is waited for.
    ovs_status edge_chi2_dev(ovs_ba_graph* g, const std::vector<Pose>& T, double* d_chi_judged) {
        ovs_status st = upload_poses(T, d_poses, nullptr);
        if (st != OVS_OK) return st;
        if (err_at_trial) {
            st = ovs::ba_graph_edge_chi2(g, d_poses_n, d_Xn, d_chi_judged, d_edepth, stream);
            if (st != OVS_OK) return st;
        }
        return ovs::ba_graph_edge_chi2(g, d_poses, d_X, err_at_trial ? d_echi_s : d_chi_judged, d_edepth, stream);
    }
    // after round 1: flags into d_out1, the graph's active mask, the number of inliers (one 4-byte download and the wait for it)
    ovs_status gate_round1(ovs_ba_graph* g, const std::vector<Pose>& T, size_t ne, size_t* n_act) {
        *n_act = 0;
        if (ne == 0) return OVS_OK;
        OVS_HIP_TRY(hipMemsetAsync(d_nact, 0, sizeof(int32_t), stream));
        ovs_status st = edge_chi2_dev(g, T, d_echi_r1);
        if (st != OVS_OK) return st;
        st = ovs::ba_graph_edge_gate(g, kChi2D, kChi3D, d_echi_r1, d_edepth, nullptr, nullptr, false, d_out1, true, d_nact, stream);
        if (st != OVS_OK) return st;
        int32_t* const h_n = reinterpret_cast<int32_t*>(h_edge);
        OVS_HIP_TRY(hipMemcpyAsync(h_n, d_nact, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
        OVS_HIP_TRY(hipStreamSynchronize(stream));
        *n_act = (size_t)*h_n;
        return OVS_OK;
    }
    // the final flags (ne bytes, into the page-locked block) and the landmarks (into h_pts) in one wait
    ovs_status gate_final(ovs_ba_graph* g, const std::vector<Pose>& T, size_t ne, bool round2_ran, const uint8_t*& flags) {
        flags = h_edge;
        if (ne) {
            ovs_status st = edge_chi2_dev(g, T, d_echi);
            if (st != OVS_OK) return st;
            st = ovs::ba_graph_edge_gate(g, kChi2D, kChi3D, d_echi, d_edepth, d_echi_r1, d_out1, round2_ran, d_outf, false, nullptr, stream);
            if (st != OVS_OK) return st;
            OVS_HIP_TRY(hipMemcpyAsync(h_edge, d_outf, ne, hipMemcpyDeviceToHost, stream));
        }
        OVS_HIP_TRY(hipMemcpyAsync(h_pts, d_X, sizeof(double) * 3 * (size_t)n_pt, hipMemcpyDeviceToHost, stream));
        OVS_HIP_TRY(hipStreamSynchronize(stream));
        return OVS_OK;
    }
};

struct GraphGuard {
    ovs_ba_graph* g = nullptr;
    ~GraphGuard() {
        if (g) ovs_ba_graph_destroy(g);
    }
};

}   // namespace

// model 0: perspective (ovs_ba_graph_create), model 1: equirectangular (cam = {cols, rows, -, -}, mono edges only)
static ovs_status local_ba_optimize_impl(int model, int32_t device, double* poses, const uint8_t* pose_fixed, int32_t n_pose, double* points,
                                         int32_t n_pt, const ovs_ba_edge* mono, int32_t n_mono, const ovs_ba_edge_stereo* stereo, int32_t n_stereo,
                                         const ovs_ba_cam* cam, double focal_x_baseline, int32_t setup_type, int32_t num_first_iter,
                                         int32_t num_second_iter, const volatile uint8_t* force_stop_flag, uint8_t* mono_outlier,
                                         uint8_t* stereo_outlier, double* info) {
    if (!poses || !points || !cam || n_pose < 1 || n_pt < 1 || n_mono < 0 || n_stereo < 0 || (n_mono > 0 && (!mono || !mono_outlier)) ||
        (n_stereo > 0 && (!stereo || !stereo_outlier)) || num_first_iter < 0 || num_second_iter < 0)
        return OVS_ERR_INVALID;
    if (ovs_device_count() <= device || device < 0) return OVS_ERR_NO_DEVICE;
    OVS_HIP_TRY(hipSetDevice(device));
    // ---- the work space first (round 6): the landmarks' upload is on its way while the host indexes the edges
    const bool trace = ovs::tuning().ba_trace;
    const double t_begin = Lm::now();
    const size_t ne = (size_t)n_mono + n_stereo;
    Lm L;
    L.setup_type = setup_type;
    ovs_status st = L.init(device, n_pose, n_pt, ne, points);
    if (st != OVS_OK) return st;
    // ---- round 1 graph: all edges (validates the indices)
    GraphGuard g1;
    st = model == 1 ? ovs_ba_graph_create_equirect(device, n_pose, pose_fixed, n_pt, mono, n_mono, (int32_t)cam->fx, (int32_t)cam->fy, &g1.g)
                    : ovs_ba_graph_create(device, n_pose, pose_fixed, n_pt, mono, n_mono, stereo, n_stereo, cam, focal_x_baseline, &g1.g);
    if (st != OVS_OK) {
        (void)hipStreamSynchronize(L.stream);   // (the landmarks' upload reads the thread's page-locked block)
        return st;
    }
    const double t_g1 = Lm::now();
    std::vector<Pose> T((size_t)n_pose);
    for (int k = 0; k < n_pose; ++k) {
        quat_to_rot(poses + 7 * (size_t)k + 3, T[k].R);
        for (int a = 0; a < 3; ++a) T[k].t[a] = poses[7 * (size_t)k + a];
    }
    double info_l[6] = {0, 0, 0, 0, 0, 0};
    int it1 = 0, it2 = 0;
    if (ne == 0) num_first_iter = num_second_iter = 0;
    st = L.run_round(g1.g, T, num_first_iter, true, force_stop_flag, &info_l[0], &info_l[1], &it1);
    if (st != OVS_OK) return st;
    const double t_r1 = Lm::now();
    // ---- the chi-square gates on the device (k_edge_gate, round 6): the per-edge arrays stay in HBM, the active mask is written where
    //      round 2 reads it, 4 bytes come down after round 1 and the flags (one byte per edge) at the end
    size_t n_act = 0;
    st = L.gate_round1(g1.g, T, ne, &n_act);
    if (st != OVS_OK) return st;
    const double t_gate1 = Lm::now();
    const bool stopped = force_stop_flag && *force_stop_flag;
    if (!stopped) {
        // ---- round 2: inliers only (outliers go to level 1), no robust kernel. The graph is kept: level-1 edges are masked, they then
        //      contribute exact zeros and the sums over the remaining edges keep their order -- the result a rebuilt graph would give
        st = L.run_round(g1.g, T, n_act ? num_second_iter : 0, false, force_stop_flag, &info_l[2], &info_l[3], &it2);
        if (st != OVS_OK) return st;
    }
    const double t_r2 = Lm::now();
    const uint8_t* flags = nullptr;
    st = L.gate_final(g1.g, T, ne, !stopped, flags);
    if (st != OVS_OK) return st;
    if (n_mono > 0) std::memcpy(mono_outlier, flags, (size_t)n_mono);
    if (n_stereo > 0) std::memcpy(stereo_outlier, flags + n_mono, (size_t)n_stereo);
    std::vector<double> p7;
    Lm::pack_poses(T, p7);
    for (int k = 0; k < n_pose; ++k)
        if (!(pose_fixed && pose_fixed[k])) std::memcpy(poses + 7 * (size_t)k, &p7[(size_t)7 * k], sizeof(double) * 7);
    std::memcpy(points, L.h_pts, sizeof(double) * 3 * (size_t)n_pt);
    if (trace)
        std::fprintf(stderr, "[ovs_local_ba_optimize] total %.2f ms: work space + graph build %.2f, round 1 %.2f, gates %.2f, round 2 %.2f, final gates + "
                             "download %.2f; %d trials: schur+download %.2f, host cholesky %.2f, update+linearise (device solver: the whole trial) %.2f ms\n",
                     Lm::now() - t_begin, t_g1 - t_begin, t_r1 - t_g1, t_gate1 - t_r1, t_r2 - t_gate1, Lm::now() - t_r2, L.n_trials, L.t_schur, L.t_chol,
                     L.t_trial);
    if (info) {
        info_l[4] = it1;
        info_l[5] = it2;
        std::memcpy(info, info_l, sizeof(info_l));
    }
    return OVS_OK;
}

// optimize::global_bundle_adjuster::optimize behind the flattening: every keyframe and landmark, ONE optimizer.optimize(num_iter) round, Huber
// kernels with the caller's deltas, no outlier gates. With solver 1 the launches are those of local BA's first round.
static ovs_status global_ba_optimize_impl(int model, int32_t device, double* poses, const uint8_t* pose_fixed, int32_t n_pose, double* points, int32_t n_pt,
                                          const ovs_ba_edge* mono, int32_t n_mono, const ovs_ba_edge_stereo* stereo, int32_t n_stereo, const ovs_ba_cam* cam,
                                          double focal_x_baseline, double huber_mono, double huber_stereo, int32_t num_iter, int32_t solver,
                                          const volatile uint8_t* force_stop_flag, double* info) {
    if (!poses || !points || !cam || n_pose < 1 || n_pt < 1 || n_mono < 0 || n_stereo < 0 || (n_mono > 0 && !mono) || (n_stereo > 0 && !stereo) ||
        num_iter < 0 || solver < 0 || solver > 2 || !(huber_mono >= 0.0 && huber_mono < __builtin_inf()) ||
        !(huber_stereo >= 0.0 && huber_stereo < __builtin_inf()))
        return OVS_ERR_INVALID;
    // ---- the solver, by the number of free keyframes alone: before the device and any allocation
    int n_free = 0;
    for (int k = 0; k < n_pose; ++k) n_free += (pose_fixed && pose_fixed[k]) ? 0 : 1;
    const int n = 6 * n_free;
    const int used = solver != 0 ? solver : n <= ovs::dense_solve_max_n() ? 1 : 2;
    if (used == 1 ? n > ovs::dense_solve_max_n() : n_free > ovs::pcg_max_free()) return OVS_ERR_CAPACITY;
    if (ovs_device_count() <= device || device < 0) return OVS_ERR_NO_DEVICE;
    OVS_HIP_TRY(hipSetDevice(device));
    const size_t ne = (size_t)n_mono + n_stereo;
    Lm L;
    L.huber_given = true;
    L.huber_mono_given = huber_mono;
    L.huber_stereo_given = huber_stereo;
    ovs_status st = L.init(device, n_pose, n_pt, ne, points, false);
    if (st != OVS_OK) return st;
    GraphGuard g1;
    st = model == 1 ? ovs_ba_graph_create_equirect(device, n_pose, pose_fixed, n_pt, mono, n_mono, (int32_t)cam->fx, (int32_t)cam->fy, &g1.g)
                    : ovs_ba_graph_create(device, n_pose, pose_fixed, n_pt, mono, n_mono, stereo, n_stereo, cam, focal_x_baseline, &g1.g);
    if (st != OVS_OK) {
        (void)hipStreamSynchronize(L.stream);   // (the landmarks' upload reads the thread's page-locked block)
        return st;
    }
    std::vector<Pose> T((size_t)n_pose);
    for (int k = 0; k < n_pose; ++k) {
        quat_to_rot(poses + 7 * (size_t)k + 3, T[k].R);
        for (int a = 0; a < 3; ++a) T[k].t[a] = poses[7 * (size_t)k + a];
    }
    double chi0 = 0, chi1 = 0;
    int it = 0;
    st = L.run_round(g1.g, T, ne == 0 ? 0 : num_iter, true, force_stop_flag, &chi0, &chi1, &it, used);
    if (st != OVS_OK) return st;
    if (L.n_accepted > 0) {   // (no accepted trial: the caller's arrays keep their bits, a quaternion is not taken through a matrix and back)
        OVS_HIP_TRY(hipMemcpyAsync(L.h_pts, L.d_X, sizeof(double) * 3 * (size_t)n_pt, hipMemcpyDeviceToHost, L.stream));
        OVS_HIP_TRY(hipStreamSynchronize(L.stream));
        std::vector<double> p7;
        Lm::pack_poses(T, p7);
        for (int k = 0; k < n_pose; ++k)
            if (!(pose_fixed && pose_fixed[k])) std::memcpy(poses + 7 * (size_t)k, &p7[(size_t)7 * k], sizeof(double) * 7);
        std::memcpy(points, L.h_pts, sizeof(double) * 3 * (size_t)n_pt);
    }
    if (info) {
        const double out[8] = {chi0, chi1, (double)it, (double)L.n_trials, (double)used, (double)L.pcg_iterations, (double)L.pcg_capped, (double)L.failed_solves};
        std::memcpy(info, out, sizeof(out));
    }
    return OVS_OK;
}

extern "C" {

ovs_status ovs_global_ba_optimize(int32_t device, double* poses, const uint8_t* pose_fixed, int32_t n_pose, double* points, int32_t n_pt,
                                  const ovs_ba_edge* mono, int32_t n_mono, const ovs_ba_edge_stereo* stereo, int32_t n_stereo, const ovs_ba_cam* cam,
                                  double focal_x_baseline, double huber_mono, double huber_stereo, int32_t num_iter, int32_t solver,
                                  const volatile uint8_t* force_stop_flag, double* info) {
    return global_ba_optimize_impl(0, device, poses, pose_fixed, n_pose, points, n_pt, mono, n_mono, stereo, n_stereo, cam, focal_x_baseline, huber_mono,
                                   huber_stereo, num_iter, solver, force_stop_flag, info);
}

ovs_status ovs_global_ba_optimize_equirect(int32_t device, double* poses, const uint8_t* pose_fixed, int32_t n_pose, double* points, int32_t n_pt,
                                           const ovs_ba_edge* mono, int32_t n_mono, int32_t cols, int32_t rows, double huber_mono, int32_t num_iter,
                                           int32_t solver, const volatile uint8_t* force_stop_flag, double* info) {
    if (cols < 1 || rows < 1) return OVS_ERR_INVALID;
    const ovs_ba_cam cam = {(double)cols, (double)rows, 0.0, 0.0};
    return global_ba_optimize_impl(1, device, poses, pose_fixed, n_pose, points, n_pt, mono, n_mono, nullptr, 0, &cam, 0.0, huber_mono, 0.0, num_iter, solver,
                                   force_stop_flag, info);
}

ovs_status ovs_local_ba_optimize(int32_t device, double* poses, const uint8_t* pose_fixed, int32_t n_pose, double* points, int32_t n_pt,
                                 const ovs_ba_edge* mono, int32_t n_mono, const ovs_ba_edge_stereo* stereo, int32_t n_stereo,
                                 const ovs_ba_cam* cam, double focal_x_baseline, int32_t setup_type, int32_t num_first_iter, int32_t num_second_iter,
                                 const volatile uint8_t* force_stop_flag, uint8_t* mono_outlier, uint8_t* stereo_outlier, double* info) {
    return local_ba_optimize_impl(0, device, poses, pose_fixed, n_pose, points, n_pt, mono, n_mono, stereo, n_stereo, cam, focal_x_baseline, setup_type,
                                  num_first_iter, num_second_iter, force_stop_flag, mono_outlier, stereo_outlier, info);
}

ovs_status ovs_local_ba_set_solver(int32_t where) {
    if (where != 0 && where != 1) return OVS_ERR_INVALID;
    ovs::g_lba_solver.store(where, std::memory_order_relaxed);
    return OVS_OK;
}
int32_t ovs_local_ba_get_solver(void) { return ovs::g_lba_solver.load(std::memory_order_relaxed); }

ovs_status ovs_local_ba_optimize_equirect(int32_t device, double* poses, const uint8_t* pose_fixed, int32_t n_pose, double* points, int32_t n_pt,
                                          const ovs_ba_edge* mono, int32_t n_mono, int32_t cols, int32_t rows, int32_t num_first_iter,
                                          int32_t num_second_iter, const volatile uint8_t* force_stop_flag, uint8_t* mono_outlier, double* info) {
    if (cols < 1 || rows < 1) return OVS_ERR_INVALID;
    const ovs_ba_cam cam = {(double)cols, (double)rows, 0.0, 0.0};
    return local_ba_optimize_impl(1, device, poses, pose_fixed, n_pose, points, n_pt, mono, n_mono, nullptr, 0, &cam, 0.0, 0, num_first_iter,
                                  num_second_iter, force_stop_flag, mono_outlier, nullptr, info);
}

}   // extern "C"
