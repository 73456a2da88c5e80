// pose_plan.inc -- the launch plan of the pose optimiser (pose_opt.hip): which form of k_pose_optimize a call runs, and where the sections of the
// staged block of a one-frame call lie. Plain integer host code, no HIP: pose_opt.hip includes it for its two host functions, tests/pose_plan_host.cc
// builds it with the host compiler alone (tests/test_pose_plan.py holds it to a table). This is the one place the launch form is decided.
#include <algorithm>
#include <cstddef>

namespace ovs {

constexpr int kPoseMaxObs = 8192;    // <= 32 observations per thread: the inlier flags of a thread fit one register
constexpr int kPoseMaxGroups = 8;    // workgroups one frame is spread over, at most: one XCD's share of an 8 G-workgroup launch
constexpr int kPoseExchangeWords = 2 * kPoseMaxGroups * 56;   // 64-bit words of a frame's exchange buffer: two epochs x groups x 28 doubles in halves
constexpr size_t kPoseObsBytes = 64;   // sizeof(ovs_pose_obs)

struct PoseSwitches {   // the environment's say (Tuning: pose_threads, pose_groups, pose_batch_retries, pose_obs_regs, pose_zero_copy)
    int threads, groups, batch_retries;   // 0 / 0 / -1 = by problem size
    bool obs_regs, zero_copy;
};

struct PoseLaunch {
    int threads, groups, batch_retries;   // k_pose_optimize<MODEL, threads, kreg>, G, retries 1 .. 9 of an iteration in one pass
    int kreg;                             // 2 = no thread owns more than two observations: their records are held in registers; 0 = re-read per pass
    bool zero_copy;                       // the kernel reads and writes the pinned host block itself: no copy before or after it
};

// One frame of n observations through the host entry (model 0 perspective, 1 equirectangular). first_attempt = false: the frame's workgroups did not
// all become resident within the barrier's 50 ms (num_valid == -2), the frame runs again in one workgroup, inputs through device memory.
inline PoseLaunch pose_plan_frame(int model, int n, const PoseSwitches& s, bool first_attempt) {
    PoseLaunch l;
    // workgroups: profiles/r06w_pose_groups.txt (2 from 500, 4 from 850, 8 from 1600 observations; earlier: r04w_, r05s_pose_groups.txt)
    l.groups = !first_attempt ? 1 : s.groups > 0 ? std::min(s.groups, kPoseMaxGroups) : (n >= 1600 ? 8 : n >= 850 ? 4 : n >= 500 ? 2 : 1);
    // one latency-bound workgroup: 512 threads hide the f64 latency of the per-observation work once there is enough of it (DESIGN.md 3.7)
    const int by_size = l.groups > 1 ? 256 : ((model == 1 ? n >= 1500 : n >= 768) ? 512 : 256);
    l.threads = s.threads == 256 || s.threads == 512 ? s.threads : by_size;
    // nine trial poses per observation pay where a thread holds few observations: profiles/r04aj_pose_batched_retries.txt
    l.batch_retries = s.batch_retries == 0 || s.batch_retries == 1 ? s.batch_retries : ((l.groups > 1 || n <= 512) ? 1 : 0);
    // records in registers: 256-thread workgroups only, and only where the size alone would have chosen them (a forced 256 above the 512-thread
    // threshold re-reads its records, as a forced 512 does)
    l.kreg = (n <= 2 * l.groups * 256 && by_size == 256 && l.threads == 256 && s.obs_regs) ? 2 : 0;
    l.zero_copy = l.kreg && s.zero_copy && first_attempt;
    return l;
}

// The two batch entries: one workgroup per frame, records and results in the caller's device memory, frames of any size side by side.
inline PoseLaunch pose_plan_batch(const PoseSwitches& s) {
    PoseLaunch l;
    l.threads = s.threads == 512 ? 512 : 256;
    l.groups = 1;
    l.batch_retries = s.batch_retries == 1 ? 1 : 0;
    l.kreg = 0;
    l.zero_copy = false;
    return l;
}

// The staged block of a one-frame call and its pinned host mirror: inputs [pose 12 f64 | offsets 2 i32 | 16 bytes unused | observations] go up in
// ONE copy, outputs [pose 12 f64 | num_valid | pad | outlier flags] come back in ONE copy (or neither, PoseLaunch::zero_copy); the exchange words
// of the grouped form follow, in device memory only.
struct PoseBlock {
    size_t off_off, off_obs, in_bytes, off_out, off_nv, off_fl, out_bytes, off_part, total;
};
inline PoseBlock pose_block_of(int n_obs) {
    const size_t no = (size_t)std::max(n_obs, 1);
    PoseBlock b;
    b.off_off = 96;
    b.off_obs = 128;   // (64-byte records on a 64-byte boundary)
    b.in_bytes = b.off_obs + kPoseObsBytes * no;
    b.off_out = (b.in_bytes + 255) & ~(size_t)255;
    b.off_nv = b.off_out + 96;
    b.off_fl = b.off_out + 128;
    b.out_bytes = 128 + no;
    b.off_part = (b.off_out + b.out_bytes + 255) & ~(size_t)255;
    b.total = b.off_part + sizeof(unsigned long long) * kPoseExchangeWords;
    return b;
}

}   // namespace ovs
