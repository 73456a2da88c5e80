// The pose optimiser's launch plan (openvslam_amd/csrc/pose_plan.inc) as a stand-alone host program: no device, no library, the plain host compiler.
// usage: pose_plan_host ROW...   one line of output per row, read by tests/test_pose_plan.py:
//   frame:MODEL:N:THREADS:GROUPS:RETRIES:OBS_REGS:ZERO_COPY:FIRST  ->  threads groups batch_retries kreg zero_copy     (pose_plan_frame)
//   batch:THREADS:GROUPS:RETRIES:OBS_REGS:ZERO_COPY                ->  threads groups batch_retries kreg zero_copy     (pose_plan_batch)
//   block:N                                                        ->  off_off off_obs in_bytes off_out off_nv off_fl out_bytes off_part total
// THREADS, GROUPS, RETRIES are the switches as Tuning holds them (0, 0, -1 = by problem size); the others 0 / 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pose_plan.inc"

static bool fields(const char* row, const char* kind, size_t want, std::vector<int>& v) {
    const size_t k = std::strlen(kind);
    if (std::strncmp(row, kind, k) != 0 || row[k] != ':') return false;
    v.clear();
    for (const char* at = row + k; *at == ':';) {
        char* end = nullptr;
        v.push_back((int)std::strtol(at + 1, &end, 10));
        if (end == at + 1) return false;
        at = end;
    }
    return v.size() == want;
}

static void print(const ovs::PoseLaunch& l) { std::printf("%d %d %d %d %d\n", l.threads, l.groups, l.batch_retries, l.kreg, l.zero_copy ? 1 : 0); }

int main(int argc, char** argv) {
    std::vector<int> v;
    for (int i = 1; i < argc; ++i) {
        if (fields(argv[i], "frame", 8, v)) {
            print(ovs::pose_plan_frame(v[0], v[1], ovs::PoseSwitches{v[2], v[3], v[4], v[5] != 0, v[6] != 0}, v[7] != 0));
        } else if (fields(argv[i], "batch", 5, v)) {
            print(ovs::pose_plan_batch(ovs::PoseSwitches{v[0], v[1], v[2], v[3] != 0, v[4] != 0}));
        } else if (fields(argv[i], "block", 1, v)) {
            const ovs::PoseBlock b = ovs::pose_block_of(v[0]);
            std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", b.off_off, b.off_obs, b.in_bytes, b.off_out, b.off_nv, b.off_fl, b.out_bytes, b.off_part, b.total);
        } else {
            return 2;
        }
    }
    return 0;
}
