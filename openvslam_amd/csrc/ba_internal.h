// ba_internal.h -- what the local-BA translation units (ba_graph.hip, ba_solve.hip, ba_optimize.hip, ba_linearize.hip) share: the functions
// one unit defines for another, the launch check, and the two helpers their arenas and page-locked blocks are built with.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstddef>

#include "ovs_common.h"

#define OVS_LAUNCH_TRY(name)                                  \
    do {                                                      \
        hipError_t _e = hipGetLastError();                    \
        if (_e != hipSuccess) {                               \
            ovs::set_last_error("launch of " name, _e);       \
            return OVS_ERR_HIP;                               \
        }                                                     \
    } while (0)

struct ovs_ba_graph;

namespace ovs {

// ---- ba_graph.hip: Levenberg-Marquardt on top of a graph (comments at the definitions)
ovs_status ba_graph_ensure_solver(ovs_ba_graph* g, hipStream_t s);
ovs_status ba_graph_reset_system(ovs_ba_graph* g, hipStream_t s);
ovs_status ba_graph_schur(ovs_ba_graph* g, const double* d_Hpp, const double* d_bp, const double* d_Hll, const double* d_bl, const double* d_Hpl,
                          double lambda, hipStream_t s, int fail_word, bool clear_first);
ovs_status ba_graph_backsub(ovs_ba_graph* g, const double* d_Hpl, const double* d_bl, double lambda, const double* d_X, double* d_Xn, hipStream_t s);
ovs_status ba_graph_edge_chi2(ovs_ba_graph* g, const double* d_poses, const double* d_points, double* d_chi, uint8_t* d_depth, hipStream_t s);
ovs_status ba_graph_edge_gate(ovs_ba_graph* g, double thr_mono, double thr_stereo, const double* d_chi, const uint8_t* d_depth, const double* d_chi_r1,
                              const uint8_t* d_out1, bool use_final, uint8_t* d_out, bool write_active, int32_t* d_n_active, hipStream_t s);
ovs_status ba_graph_linearize(ovs_ba_graph* g, const double* d_poses, const double* d_points, double huber_mono, double huber_stereo, double* d_Hpp,
                              double* d_bp, double* d_Hll, double* d_bl, double* d_Hpl, double* d_chi3, hipStream_t s, double* d_chi_mirror = nullptr,
                              bool trial_scale = false, unsigned long long* host_ll = nullptr, unsigned int seq = 0);
ovs_status ba_graph_trial_update(ovs_ba_graph* g, const double* d_T, const double* d_bp, const double* d_Hpl, const double* d_bl, double lambda,
                                 double* d_Tn, double* d_p7n, const double* d_X, double* d_Xn, hipStream_t s, int next_fail_word);
struct BaGraphInfo {
    int n_free;
    const int32_t* slot;            // pose -> reduced block or -1 (host)
    double *d_S, *d_dxp, *d_scal;   // S | rhs | bp copy;  6 per keyframe;  [0] landmarks' / [1] keyframes' part of the gain ratio's denominator
    int32_t* d_fail;                // two failure words, 256 bytes behind d_scal
    const int32_t* d_slot_of_pose;
    int s_pitch;                    // doubles per row of d_S (6 n_free rounded up to 16; ba_solve.hip's padded layout)
    double* d_rhs;                  // row s_pitch of the system
};
BaGraphInfo ba_graph_info(ovs_ba_graph* g);

// ---- ba_solve.hip: the dense solver and the padded layout of the reduced camera system
int dense_solve_max_n();
int dense_solve_pad(int n);
size_t dense_solve_doubles(int n);
ovs_status launch_dense_solve(double* d_S, int n, int32_t* d_fail, hipStream_t s, unsigned long long* d_tstats = nullptr);

// ---- ba_optimize.hip: where the reduced camera system is solved: 0 = on the device (k_chol_solve), 1 = on the host (ba_host_math.h cholesky_solve)
extern std::atomic<int> g_lba_solver;

// One allocation, many arrays: offsets in placement order, each 256-byte aligned (an empty array still takes a byte, so no two share an offset).
struct ArenaLayout {
    size_t top = 0;
    template <class T>
    size_t place(size_t count) {
        const size_t off = bytes();
        top = off + std::max<size_t>(sizeof(T) * count, 1);
        return off;
    }
    size_t bytes() const { return (top + 255) & ~(size_t)255; }   // where the next array would start = the size to allocate
    template <class T>
    static T* at(void* base, size_t off) {
        return reinterpret_cast<T*>(static_cast<unsigned char*>(base) + off);
    }
};

// A page-locked block that only grows (per-thread work space: hipHostMalloc / hipHostFree per call cost more than the copies they serve).
// `grow_to`: what to allocate when `need` does not fit -- the caller's head room.
struct PinnedBuffer {
    unsigned char* p = nullptr;
    size_t cap = 0;   // bytes
    PinnedBuffer() = default;
    PinnedBuffer(const PinnedBuffer&) = delete;
    PinnedBuffer& operator=(const PinnedBuffer&) = delete;
    ~PinnedBuffer() { release(); }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
    hipError_t ensure(size_t need, size_t grow_to) {
        if (cap >= need) return hipSuccess;
        release();
        const hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p), grow_to, hipHostMallocDefault);
        if (e == hipSuccess) cap = grow_to;
        else p = nullptr;
        return e;
    }
};

}   // namespace ovs
