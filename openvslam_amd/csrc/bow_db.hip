// bow_db.hip -- data::bow_database (expected: src/openvslam/data/bow_database.{h,cc}): the scoring half of acquire_loop_candidates /
// acquire_relocalization_candidates. Upstream walks an inverted file word -> keyframes on the host to find the keyframes sharing a word
// with the query, then calls DBoW2's L1Scoring::score on each; here every registered keyframe's BowVector is resident in HBM and ONE launch
// scores all of them (rules 1 to 3; rules 4 to 6 run on the host over the survivors).
//
// Layout: slot s of the handle owns row s of two arrays, ids [max_keyframes][max_words] int32 and values [..][..] f64, plus a 16-byte
// record (length, keyframe id, live). The query (ids + values, 12 B per word) is staged once per workgroup in LDS.
//
// k_bowdb_score: one wavefront per slot, slots dealt round-robin to the waves of a grid sized to the device (not to the database: the
// launch count is two whatever the number of keyframes). The lanes take the keyframe's entries lane + 64 r in rounds; every lane finds
// its word among the query's ids by a branch-free binary search in LDS and, on a hit, computes its own term
// (fabs(qv - kv) - fabs(qv)) - fabs(kv). Within a round the hits are ascending by lane and the rounds are ascending, so walking the
// ballot of hits and adding the read-lane terms onto a wave-uniform accumulator adds them in ascending word id, one after the other:
// the bits of the sequential merge loop. The dependent chain is one f64 add per common word. Integer atomicMax for max_common; no
// floating-point atomics anywhere.
// k_bowdb_gate: one thread per slot; the survivors of the common-word gate (or, for score_all, every live slot) go to page-locked
// arrays through an integer ticket, the host sorts the short list by keyframe id.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <numeric>
#include <unordered_map>
#include <vector>

#include "ovs_common.h"
#include "owned_internal.inc"

namespace {

struct SlotRec {
    int32_t len, keyframe_id, live, pad;
};
static_assert(sizeof(SlotRec) == 16, "SlotRec is read as one 128-bit word");

// the head of the staged query block: the two words the launches reduce into, zeroed by the same copy that brings the query
struct QueryHead {
    int32_t max_common, n_out, pad0, pad1;
};

constexpr int kWavesPerGroup = 4;

}   // namespace

struct ovs_bowdb {
    int device = 0;
    int max_keyframes = 0, max_words = 0, n_cu = 0;
    std::mutex mu;
    ovs::Owned res;
    hipStream_t stream = nullptr;
    // database
    int32_t* d_ids = nullptr;
    double* d_vals = nullptr;
    SlotRec* d_slots = nullptr;
    // per query: staged block [QueryHead | values nq f64 | ids nq i32 | rejected slots n_reject i32], page-locked twin of the same layout
    uint8_t *d_query = nullptr, *h_query = nullptr;
    size_t query_cap = 0;
    int32_t* d_common = nullptr;    // per slot
    double* d_score = nullptr;      // per slot
    uint8_t* d_rejected = nullptr;  // per slot
    // results, page-locked and mapped: the gate kernel writes them, the host reads them after the stream has drained
    int32_t *h_out_id = nullptr, *h_out_common = nullptr;
    double* h_out_score = nullptr;
    QueryHead* h_head = nullptr;
    int32_t *m_out_id = nullptr, *m_out_common = nullptr;   // the device's view of the three result arrays
    double* m_out_score = nullptr;
    // host bookkeeping
    std::unordered_map<int32_t, int32_t> slot_of;   // keyframe id -> slot
    std::vector<int32_t> free_slots;                // erased slots below `hi`, reused before the database grows
    int32_t hi = 0;                                 // slots [0, hi) have been used
    std::vector<int32_t> order;
};

namespace {

__global__ __launch_bounds__(64 * kWavesPerGroup) void k_bowdb_score(const int32_t* __restrict__ ids, const double* __restrict__ vals,
                                                                    const SlotRec* __restrict__ slots, int max_words, int n_slots,
                                                                    uint8_t* query, int nq, int n_reject,
                                                                    int32_t* __restrict__ out_common, double* __restrict__ out_score,
                                                                    uint8_t* __restrict__ out_rejected) {
    extern __shared__ double lds[];
    double* q_val = lds;                                        // nq
    int32_t* q_id = reinterpret_cast<int32_t*>(lds + nq);       // nq
    const double* g_val = reinterpret_cast<const double*>(query + sizeof(QueryHead));
    const int32_t* g_id = reinterpret_cast<const int32_t*>(g_val + nq);
    const int32_t* g_rej = g_id + nq;
    for (int i = threadIdx.x; i < nq; i += blockDim.x) {
        q_val[i] = g_val[i];
        q_id[i] = g_id[i];
    }
    __syncthreads();
    int top = 0;   // largest power of two <= nq: the first stride of the binary search
    if (nq > 0) top = 1 << (31 - __clz(nq));
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWavesPerGroup + (threadIdx.x >> 6)));
    const int n_waves = gridDim.x * kWavesPerGroup;
    int* max_common = &reinterpret_cast<QueryHead*>(query)->max_common;
    for (int slot = wave; slot < n_slots; slot += n_waves) {
        const SlotRec rec = slots[slot];
        if (!rec.live) continue;   // wave-uniform
        bool rejected = false;
        for (int i = lane; i < n_reject; i += 64) rejected |= g_rej[i] == slot;
        rejected = __ballot(rejected) != 0;
        const int32_t* kid = ids + (size_t)slot * max_words;
        const double* kval = vals + (size_t)slot * max_words;
        const int len = rec.len;
        double s = 0.0;
        int common = 0;
        int32_t id_next = 0;
        double kv_next = 0.0;
        if (lane < len) {
            id_next = kid[lane];
            kv_next = kval[lane];
        }
        for (int base = 0; base < len; base += 64) {
            const int32_t id = id_next;
            const double kv = kv_next;
            const bool valid = base + lane < len;
            if (base + 64 + lane < len) {   // the next round's entries are in flight while this round searches
                id_next = kid[base + 64 + lane];
                kv_next = kval[base + 64 + lane];
            }
            int pos = 0;   // number of query ids below `id`
            for (int step = top; step; step >>= 1) {
                const int t = pos + step;
                if (t <= nq && q_id[t - 1] < id) pos = t;
            }
            const bool hit = valid && pos < nq && q_id[pos] == id;
            double term = 0.0;
            if (hit) {
                const double qv = q_val[pos];
                term = (fabs(qv - kv) - fabs(qv)) - fabs(kv);
            }
            unsigned long long m = __ballot(hit);
            common += __popcll(m);
            const int t_lo = __double2loint(term), t_hi = __double2hiint(term);
            while (m) {   // ascending lane = ascending word id
                const int l = __builtin_ctzll(m);
                m &= m - 1;
                s += __hiloint2double(__builtin_amdgcn_readlane(t_hi, l), __builtin_amdgcn_readlane(t_lo, l));
            }
        }
        if (lane == 0) {
            out_common[slot] = common;
            out_score[slot] = common ? -s / 2.0 : 0.0;
            out_rejected[slot] = rejected ? 1 : 0;
            if (common && !rejected) atomicMax(max_common, common);
        }
    }
}

__global__ __launch_bounds__(256) void k_bowdb_gate(const SlotRec* __restrict__ slots, int n_slots, const int32_t* __restrict__ common,
                                                   const double* __restrict__ score, const uint8_t* __restrict__ rejected,
                                                   uint8_t* __restrict__ query, int all, int32_t* __restrict__ out_id,
                                                   int32_t* __restrict__ out_common, double* __restrict__ out_score) {
    const int slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= n_slots) return;
    const SlotRec rec = slots[slot];
    if (!rec.live) return;
    QueryHead* head = reinterpret_cast<QueryHead*>(query);
    const int c = common[slot];
    if (!all) {
        if (c < 1 || rejected[slot]) return;
        if (!((float)c > 0.8f * (float)head->max_common)) return;
    }
    const int at = atomicAdd(&head->n_out, 1);   // at < live slots <= max_keyframes = the arrays' size
    out_id[at] = rec.keyframe_id;
    out_common[at] = c;
    out_score[at] = score[slot];
}

ovs::LdsAttrCache g_score_lds;

// strictly ascending non-negative ids, finite values
bool vector_ok(const int32_t* ids, const double* values, int32_t n) {
    if (n < 0 || (n > 0 && (!ids || !values))) return false;
    for (int32_t i = 0; i < n; ++i) {
        if (ids[i] < 0 || (i > 0 && ids[i] <= ids[i - 1]) || !std::isfinite(values[i])) return false;
    }
    return true;
}

// Both queries: stage, score every live slot, gate, read the head back. Called with the handle's mutex held. On return h_head and the
// h_out_* arrays hold the unsorted results.
ovs_status run_query(ovs_bowdb* db, const int32_t* q_ids, const double* q_values, int32_t nq, const int32_t* reject_ids, int32_t n_reject, bool all) {
    OVS_HIP_TRY(hipSetDevice(db->device));
    QueryHead* head = reinterpret_cast<QueryHead*>(db->h_query);
    *head = QueryHead{0, 0, 0, 0};
    double* hv = reinterpret_cast<double*>(db->h_query + sizeof(QueryHead));
    int32_t* hi_ = reinterpret_cast<int32_t*>(hv + nq);
    if (nq) {
        std::memcpy(hv, q_values, sizeof(double) * (size_t)nq);
        std::memcpy(hi_, q_ids, sizeof(int32_t) * (size_t)nq);
    }
    int32_t n_rej_slots = 0;
    for (int32_t i = 0; i < n_reject; ++i) {
        const auto it = db->slot_of.find(reject_ids[i]);
        if (it != db->slot_of.end() && n_rej_slots < db->max_keyframes) hi_[nq + n_rej_slots++] = it->second;   // (duplicates beyond every slot: dropped)
    }
    db->h_head->max_common = 0;
    db->h_head->n_out = 0;
    if (db->hi == 0) return OVS_OK;
    hipStream_t s = db->stream;
    const size_t bytes = sizeof(QueryHead) + 12 * (size_t)nq + sizeof(int32_t) * (size_t)n_rej_slots;
    OVS_HIP_TRY(hipMemcpyAsync(db->d_query, db->h_query, bytes, hipMemcpyHostToDevice, s));
    const size_t lds = 12 * (size_t)std::max(nq, 1);
    OVS_HIP_TRY(ovs::ensure_dynamic_lds(reinterpret_cast<const void*>(k_bowdb_score), lds, g_score_lds));
    const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(8, (ovs::kMaxLdsPerWorkgroup) / lds));   // workgroups a CU holds: 32 waves, 160 KB
    const int groups = std::max(1, std::min((db->hi + kWavesPerGroup - 1) / kWavesPerGroup, db->n_cu * per_cu));
    hipLaunchKernelGGL(k_bowdb_score, dim3(groups), dim3(64 * kWavesPerGroup), lds, s, db->d_ids, db->d_vals, db->d_slots, db->max_words, db->hi,
                       db->d_query, nq, n_rej_slots, db->d_common, db->d_score, db->d_rejected);
    OVS_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_bowdb_gate, dim3((db->hi + 255) / 256), dim3(256), 0, s, db->d_slots, db->hi, db->d_common, db->d_score, db->d_rejected,
                       db->d_query, all ? 1 : 0, db->m_out_id, db->m_out_common, db->m_out_score);
    OVS_HIP_TRY(hipGetLastError());
    OVS_HIP_TRY(hipMemcpyAsync(db->h_head, db->d_query, sizeof(QueryHead), hipMemcpyDeviceToHost, s));
    OVS_HIP_TRY(hipStreamSynchronize(s));
    return OVS_OK;
}

// the results in ascending keyframe id into the caller's arrays
void emit_sorted(ovs_bowdb* db, int32_t n, int32_t* out_ids, int32_t* out_num_common, double* out_scores) {
    db->order.resize((size_t)n);
    std::iota(db->order.begin(), db->order.end(), 0);
    std::sort(db->order.begin(), db->order.end(), [&](int32_t a, int32_t b) { return db->h_out_id[a] < db->h_out_id[b]; });
    for (int32_t i = 0; i < n; ++i) {
        const int32_t j = db->order[(size_t)i];
        out_ids[i] = db->h_out_id[j];
        out_num_common[i] = db->h_out_common[j];
        out_scores[i] = db->h_out_score[j];
    }
}

}   // namespace

extern "C" {

ovs_status ovs_bowdb_create(int32_t device, int32_t max_keyframes, int32_t max_words, ovs_bowdb** out) {
    if (!out || max_keyframes < 1 || max_words < 1) return OVS_ERR_INVALID;
    *out = nullptr;
    if (12 * (size_t)max_words > ovs::kMaxLdsPerWorkgroup) return OVS_ERR_INVALID;   // the query has to fit one workgroup's LDS
    if (ovs_device_count() <= device || device < 0) return OVS_ERR_NO_DEVICE;
    OVS_HIP_TRY(hipSetDevice(device));
    std::unique_ptr<ovs_bowdb> owner(new ovs_bowdb());
    ovs_bowdb* const db = owner.get();
    db->device = device;
    db->max_keyframes = max_keyframes;
    db->max_words = max_words;
    db->query_cap = sizeof(QueryHead) + 12 * (size_t)max_words + sizeof(int32_t) * (size_t)max_keyframes;
    const size_t cells = (size_t)max_keyframes * (size_t)max_words;
    hipDeviceProp_t prop;
    OVS_HIP_TRY(hipGetDeviceProperties(&prop, device));
    db->n_cu = std::max(1, prop.multiProcessorCount);
    OVS_HIP_TRY(db->res.stream(&db->stream));
    OVS_HIP_TRY(db->res.dev(&db->d_ids, sizeof(int32_t) * cells));
    OVS_HIP_TRY(db->res.dev(&db->d_vals, sizeof(double) * cells));
    OVS_HIP_TRY(db->res.dev(&db->d_slots, sizeof(SlotRec) * (size_t)max_keyframes));
    OVS_HIP_TRY(hipMemset(db->d_slots, 0, sizeof(SlotRec) * (size_t)max_keyframes));
    OVS_HIP_TRY(db->res.dev(&db->d_query, db->query_cap));
    OVS_HIP_TRY(db->res.dev(&db->d_common, sizeof(int32_t) * (size_t)max_keyframes));
    OVS_HIP_TRY(db->res.dev(&db->d_score, sizeof(double) * (size_t)max_keyframes));
    OVS_HIP_TRY(db->res.dev(&db->d_rejected, (size_t)max_keyframes));
    OVS_HIP_TRY(db->res.pinned(&db->h_query, db->query_cap));
    OVS_HIP_TRY(db->res.pinned(&db->h_out_id, sizeof(int32_t) * (size_t)max_keyframes, hipHostMallocMapped));
    OVS_HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&db->m_out_id), db->h_out_id, 0));
    OVS_HIP_TRY(db->res.pinned(&db->h_out_common, sizeof(int32_t) * (size_t)max_keyframes, hipHostMallocMapped));
    OVS_HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&db->m_out_common), db->h_out_common, 0));
    OVS_HIP_TRY(db->res.pinned(&db->h_out_score, sizeof(double) * (size_t)max_keyframes, hipHostMallocMapped));
    OVS_HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&db->m_out_score), db->h_out_score, 0));
    OVS_HIP_TRY(db->res.pinned(&db->h_head, sizeof(QueryHead)));
    *out = owner.release();
    return OVS_OK;
}

ovs_status ovs_bowdb_destroy(ovs_bowdb* db) {
    if (!db) return OVS_ERR_INVALID;
    hipSetDevice(db->device);
    delete db;
    return OVS_OK;
}

ovs_status ovs_bowdb_add(ovs_bowdb* db, int32_t keyframe_id, const int32_t* word_ids, const double* values, int32_t n) {
    if (!db || !vector_ok(word_ids, values, n)) return OVS_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (db->slot_of.count(keyframe_id)) return OVS_ERR_INVALID;
    if (n > db->max_words) return OVS_ERR_CAPACITY;
    if (db->free_slots.empty() && db->hi == db->max_keyframes) return OVS_ERR_CAPACITY;
    const int32_t slot = db->free_slots.empty() ? db->hi : db->free_slots.back();
    OVS_HIP_TRY(hipSetDevice(db->device));
    hipStream_t s = db->stream;
    if (n) {
        OVS_HIP_TRY(hipMemcpyAsync(db->d_ids + (size_t)slot * db->max_words, word_ids, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s));
        OVS_HIP_TRY(hipMemcpyAsync(db->d_vals + (size_t)slot * db->max_words, values, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, s));
    }
    const SlotRec rec{n, keyframe_id, 1, 0};   // the record goes last: a slot is live only with its vector in place
    OVS_HIP_TRY(hipMemcpyAsync(db->d_slots + slot, &rec, sizeof(rec), hipMemcpyHostToDevice, s));
    OVS_HIP_TRY(hipStreamSynchronize(s));
    if (db->free_slots.empty()) ++db->hi;
    else db->free_slots.pop_back();
    db->slot_of[keyframe_id] = slot;
    return OVS_OK;
}

ovs_status ovs_bowdb_erase(ovs_bowdb* db, int32_t keyframe_id) {
    if (!db) return OVS_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    const auto it = db->slot_of.find(keyframe_id);
    if (it == db->slot_of.end()) return OVS_ERR_INVALID;
    const int32_t slot = it->second;
    OVS_HIP_TRY(hipSetDevice(db->device));
    const SlotRec rec{0, 0, 0, 0};
    OVS_HIP_TRY(hipMemcpyAsync(db->d_slots + slot, &rec, sizeof(rec), hipMemcpyHostToDevice, db->stream));
    OVS_HIP_TRY(hipStreamSynchronize(db->stream));
    db->slot_of.erase(it);
    db->free_slots.push_back(slot);
    return OVS_OK;
}

ovs_status ovs_bowdb_clear(ovs_bowdb* db) {
    if (!db) return OVS_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    OVS_HIP_TRY(hipSetDevice(db->device));
    if (db->hi) {
        OVS_HIP_TRY(hipMemsetAsync(db->d_slots, 0, sizeof(SlotRec) * (size_t)db->hi, db->stream));
        OVS_HIP_TRY(hipStreamSynchronize(db->stream));
    }
    db->slot_of.clear();
    db->free_slots.clear();
    db->hi = 0;
    return OVS_OK;
}

ovs_status ovs_bowdb_size(ovs_bowdb* db, int32_t* n) {
    if (!db || !n) return OVS_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    *n = (int32_t)db->slot_of.size();
    return OVS_OK;
}

ovs_status ovs_bowdb_query(ovs_bowdb* db, const int32_t* q_ids, const double* q_values, int32_t nq, const int32_t* reject_ids, int32_t n_reject,
                           int32_t* out_ids, int32_t* out_num_common, double* out_scores, int32_t cap, int32_t* n_out, int32_t* max_common) {
    if (!db || !n_out || !max_common || cap < 0 || n_reject < 0 || (n_reject > 0 && !reject_ids)) return OVS_ERR_INVALID;
    if (cap > 0 && (!out_ids || !out_num_common || !out_scores)) return OVS_ERR_INVALID;
    if (!vector_ok(q_ids, q_values, nq)) return OVS_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (nq > db->max_words) return OVS_ERR_CAPACITY;
    const ovs_status st = run_query(db, q_ids, q_values, nq, reject_ids, n_reject, false);
    if (st != OVS_OK) return st;
    const int32_t n = db->h_head->n_out;
    if (n > cap) return OVS_ERR_CAPACITY;   // the one error known only after the launch: nothing is written
    emit_sorted(db, n, out_ids, out_num_common, out_scores);
    *n_out = n;
    *max_common = db->h_head->max_common;
    return OVS_OK;
}

ovs_status ovs_bowdb_score_all(ovs_bowdb* db, const int32_t* q_ids, const double* q_values, int32_t nq, int32_t* out_ids, int32_t* out_num_common,
                               double* out_scores, int32_t cap, int32_t* n_out) {
    if (!db || !n_out || cap < 0) return OVS_ERR_INVALID;
    if (cap > 0 && (!out_ids || !out_num_common || !out_scores)) return OVS_ERR_INVALID;
    if (!vector_ok(q_ids, q_values, nq)) return OVS_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (nq > db->max_words || (size_t)cap < db->slot_of.size()) return OVS_ERR_CAPACITY;
    const ovs_status st = run_query(db, q_ids, q_values, nq, nullptr, 0, true);
    if (st != OVS_OK) return st;
    const int32_t n = db->h_head->n_out;
    emit_sorted(db, n, out_ids, out_num_common, out_scores);
    *n_out = n;
    return OVS_OK;
}

}   // extern "C"
