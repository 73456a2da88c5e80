// ba_pcg_internal.inc -- what ba_pcg.hip defines for ba_optimize.hip and ba_graph.hip: the conjugate-gradient solver of the reduced camera
// system for global BA (DESIGN.md 3.20; comments at the definitions). (An .inc, not an .h: see owned_internal.inc.)
#pragma once
#include "ba_internal.h"

namespace ovs {

struct PcgHostBlock {   // page-locked: what a solve brings down
    int32_t done, failed;
    double info[3];
};
struct PcgResult {
    bool failed = false, capped = false;
    int iterations = 0;
    double ratio = 0.0;   // the last dn / d0
};
int pcg_max_free();
size_t pcg_arena_bytes();
ovs_status launch_pcg_solve(const double* d_S, int pitch, double* d_rhs, int n, int32_t* d_fail, unsigned char* d_arena, PcgHostBlock* h_pin, double tol,
                            int max_iter, int check_every, hipStream_t s, PcgResult* out);
// ba_graph.hip: the solver's arena, reserved with the graph's solver work space on first use (pcg_arena_bytes())
ovs_status ba_graph_pcg_arena(ovs_ba_graph* g, unsigned char** d_arena);

}   // namespace ovs
