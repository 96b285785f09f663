// Engine state shared by the host sources — not part of the public C ABI (include/fhh.h):
//   fhh_host.cpp         one server's KeyCollection on one GPU (the engine core and its C ABI)
//   fhh_keys_io.cpp      add_keys requests in bincode: decode, append and export
//   fhh_retain.cpp       fhh_retain_clients: the collection compacted to the survivors of a keep mask
//   fhh_join.cpp         fhh_join_clients_bincode: an add_keys batch joins a ctx that has a frontier
//   fhh_sim_crawl.cpp    the in-process two-server harness: fhh_sim_*, the device-resident level loop
//   fhh_sketch_host.cpp  sketch + Beaver verification wrappers
//   fhh_group.cpp        one KeyCollection over several GPUs: clients sharded in 64-client words,
//                        per-child partials reduced over an in-process RCCL communicator
//   fhh_gcot.cpp         the GC equality test + OT extension of tree_crawl and their two-party split
//                        (each server's half on its own ctx; only byte buffers cross)
//   fhh_gcot_harness.cpp their one-shot test entry points on host buffers
#pragma once
#include "fhh_internal.h"
#include "field_arith.h"
#include "bincode_emit.h"
#include "../../include/fhh.h"

#include <hip/hip_runtime.h>

#include <array>
#include <cstdint>
#include <memory>
#include <string>
#include <utility>
#include <vector>

struct fhh_ctx;

namespace fhh {
namespace eng {

extern thread_local std::string g_err;   // message of the last failure (fhh_host.cpp)

constexpr uint64_t kFeP = (1ull << 62) - (1ull << 30) - 1;   // fastfield.rs:24-28

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    // grow-only; contents are NOT preserved
    hipError_t ensure(size_t nbytes) {
        if (nbytes <= bytes && p) return hipSuccess;
        release();
        if (nbytes == 0) nbytes = 256;
        hipError_t e = hipMalloc(&p, nbytes);
        if (e != hipSuccess) {
            p = nullptr;
            return e;
        }
        bytes = nbytes;
        return hipSuccess;
    }
    template <class T> T* as() const { return static_cast<T*>(p); }
    void swap(DevBuf& o) {
        std::swap(p, o.p);
        std::swap(bytes, o.bytes);
    }
};

struct PinnedBuf {
    void* p = nullptr;
    size_t bytes = 0;
    ~PinnedBuf() {
        if (p) (void)hipHostFree(p);
    }
    hipError_t ensure(size_t nbytes) {
        if (nbytes <= bytes && p) return hipSuccess;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        bytes = 0;
        if (nbytes == 0) nbytes = 256;
        hipError_t e = hipHostMalloc(&p, nbytes, hipHostMallocDefault);
        if (e != hipSuccess) {
            p = nullptr;
            return e;
        }
        bytes = nbytes;
        return hipSuccess;
    }
    template <class T> T* as() const { return static_cast<T*>(p); }
    void swap(PinnedBuf& o) {
        std::swap(p, o.p);
        std::swap(bytes, o.bytes);
    }
};

struct DimTable {
    DevBuf seed[2], t[2], y[2];
    size_t cap[2] = {0, 0};       // entries
    int cur = 0;                  // buffer that holds the frontier's entries
    std::vector<uint32_t> live;   // frontier entries (indices into buffer `cur`), ordered
};

struct Node {
    uint32_t pos[kMaxDims];       // position of the node's dim-j entry in tab[j].live
};

enum class Phase { kNoInit, kFrontier, kPending, kPendingLast };

// 320-bit little-endian u32 helpers for FE255 (field.rs)
using Limbs10 = std::array<uint32_t, 10>;

struct Group;       // fhh_group.cpp: shards of a multi-device ctx
struct PartyState;  // fhh_gcot.cpp: one server's half of a level's GC + OT

}  // namespace eng
}  // namespace fhh

using namespace fhh;
using namespace fhh::eng;

struct fhh_ctx {
    int device = 0;
    hipStream_t stream = nullptr;       // execution stream (own_stream, or the peer's in pair mode)
    hipStream_t own_stream = nullptr;
    fhh_ctx* peer = nullptr;            // pair mode: ctx whose staging/timing this ctx's syncs also retire
    uint32_t L = 0, d = 0, K = 0;
    uint64_t n = 0, npad = 0, nw = 0;
    uint64_t client_base = 0;
    int variant = 0;              // k_expand variant (fhh_set_variant)
    int grid = 0;
    // fhh_set_table_row_major: 1 = b = 3, 4 tables of the level loop and fhh_gt_cot*_host on k_ot_rows_out's
    // row-major labels; 0 (default, profiles/gt_tm_wide/) = the tile-major kernels
    int table_row_major = 0;
    // fhh_set_protocol_grid: >= 1 caps the grid of every GC / OT launch sized by protocol_grid (fhh_internal.h)
    // at that many workgroups; 0 (default) = the device rule. Tests and diagnostics only
    int protocol_grid = 0;
    uint32_t loop_cap_hint = 0;   // device loop: capacity the previous crawl grew to
    DevBuf work_counter;          // dynamic item distribution
    uint32_t expand_seq = 0;      // k_expand launches on work_counter (its counter slot alternates)

    // host-staged keys (add_key); uploaded at tree_init
    std::vector<uint8_t> h_key_idx, h_root, h_cws, h_cwb;
    uint64_t h_n = 0;
    bool dev_keys = false;        // keys resident on the device (uploaded or generated)

    DevBuf cw_seed, cw_bits, root_seed, key_idx, valid;
    // keys appended batch by batch (fhh_add_keys_bincode_append): until tree_init npad / nw are the layout's
    // capacity (>= n, grown geometrically), then the exact stride as on every other path
    bool appended = false;
    uint64_t reserved = 0;        // fhh_reserve_clients (0: none)
    DevBuf app_buf, app_err;      // a batch's payload and its error word, kept from call to call
    DevBuf emit_buf;              // fhh_export_keys_bincode: the serialized requests, kept from call to call
    double emit_ms = 0;           // the emit kernels' time (HIP events) of the last export here (fhh_export_timing)
    // fhh_leader_requests_ball(_device): the two servers' request bytes (handed out by the device form, valid
    // until the next such call, fhh_reset or fhh_destroy) and the call's [carry word | points | root seeds]
    DevBuf lr_out[2], lr_stage;
    // fhh_audit_keys_ball(_device): [record | ok bytes | points] of the last audit with this ctx as ctx0 (the ok
    // bytes handed out by the device form, valid until the next audit, fhh_reset or fhh_destroy), its kernel time
    // (HIP events) and its count of walks whose seeds diverged (fhh_audit_timing, fhh_audit_seed_check)
    DevBuf audit_buf;
    double audit_ms = 0;
    uint64_t audit_diverged = 0;
    // the last fhh_retain_clients that ran its kernels here: column / plane gather time (HIP events) and the
    // bytes they read plus wrote (fhh_retain_timing)
    double retain_ms[2] = {0, 0};
    uint64_t retain_bytes[2] = {0, 0};
    // fhh_retain_clients_device / fhh_retain_plan_device: [record | keep words | prefix counts] of the last mask
    // scanned here, the rows of a mask that lives on another device, and the survivor-list kernels' time (words +
    // scan, emit; HIP events), kept from call to call
    DevBuf keep_scan, keep_stage;
    double keep_ms[2] = {0, 0};
    // the last fhh_join_clients_bincode that ran its kernels here: re-pitch, decode and walk time (HIP events) and
    // the bytes the re-pitch read plus wrote (fhh_join_timing)
    double join_ms[3] = {0, 0, 0};
    uint64_t join_bytes = 0;
    DimTable tab[kMaxDims];

    Phase phase = Phase::kNoInit;
    uint32_t level = 0;           // depth of the frontier (= CorWord index of next crawl)
    std::vector<Node> frontier;
    std::vector<std::vector<std::pair<uint32_t, uint32_t>>> hist;   // per depth: (parent, i)
    uint64_t pending_C = 0;
    int child_buf[kMaxDims] = {0};
    DevBuf lists;                 // per crawl: live lists of every dim + parent_pos, one upload
    const uint32_t* live_ptr[kMaxDims] = {nullptr};
    const uint32_t* parent_pos_ptr = nullptr;   // [F][d] u32 for pending children

    // frontier_last (collect.rs:33, 909-914): surviving (parent, i) + values
    std::vector<std::pair<uint32_t, uint32_t>> last_nodes;
    std::vector<Limbs10> last_values;
    uint32_t last_depth = 0;
    std::vector<std::vector<std::pair<uint32_t, uint32_t>>> last_hist;

    DevBuf scratch, scratch2;
    // level-batched sketch verification (fhh_sim_sketch_verify_fe): a second stream for the sketch
    // tails and the verify, its events, and the odd levels' sketch outputs
    hipStream_t side_stream = nullptr;
    hipEvent_t side_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    DevBuf sketch_alt;
    DevBuf ot_buf[8], ot_rk;                     // OT extension scratch (T U Q - - Y0 Y1 choices)
    std::vector<uint32_t> ot_rk_host;            // key schedules staged for ot_rk
    std::vector<PinnedBuf*> stage;   // pinned staging for async H2D, recycled at every sync
    size_t stage_used = 0;

    fhh_stats stats{};
    bool timing = true;
    uint32_t timing_every = 1;   // device level loop: time every K-th k_expand launch
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
    std::vector<std::pair<size_t, uint64_t>> ev_pending;   // (pool index, blocks)
    size_t ev_next = 0;

    // multi-device ctx (fhh_create_multi): the shards hold the keys and the frontier; this ctx
    // only routes the KeyCollection calls (fhh_group.cpp)
    Group* group = nullptr;
    // this server's half of the current level's GC + OT when the two servers run on separate ctxs
    // (fhh_gb_* / fhh_ev_*, fhh_gcot.cpp)
    PartyState* party = nullptr;
    int party_server = -1;   // fhh_party_set_server: which server of the pair this ctx is (-1 unset), until fhh_reset

    std::string err;

    int fail(int code, const std::string& msg) {
        err = msg;
        g_err = msg;
        return code;
    }
};

// the form of ctx's equality tests for caller `who` (gt_plan.h), under its fhh_set_table_row_major switch
inline GtPlan ctx_gt_plan(const fhh_ctx* ctx, GtCaller who, uint32_t bits, uint32_t kind, uint32_t gc, bool ring_req,
                          uint64_t nw) {
    return gt_plan(who, bits, kind, gc, ring_req, ctx->table_row_major != 0, nw);
}

#define CTX_CHECK(ctx)                                              \
    do {                                                            \
        if (!(ctx)) {                                               \
            g_err = "null fhh_ctx";                                 \
            return FHH_E_ARG;                                       \
        }                                                           \
    } while (0)

#define HIP_TRY(ctx, expr)                                                                   \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return (ctx)->fail(e_ == hipErrorOutOfMemory ? FHH_E_NOMEM : FHH_E_HIP,          \
                               std::string(#expr) + ": " + hipGetErrorString(e_));          \
    } while (0)

namespace fhh {
namespace eng {

// ---- fhh_host.cpp ----------------------------------------------------------------------------
int ctx_sync(fhh_ctx* ctx);         // drain the ctx stream, retire its timing events and staging
int ctx_set_device(fhh_ctx* ctx);   // hipSetDevice(ctx->device)
ChildArgs ctx_child_args(fhh_ctx* ctx);   // the pending crawl's children as k_share_planes reads them

// what fhh_sim_crawl.cpp and fhh_keys_io.cpp take from the engine core, and fhh_tree_init from fhh_keys_io.cpp:
// between the library's own sources only, so not among its dynamic symbols
#pragma GCC visibility push(hidden)
// an event pair around what follows on the ctx stream; ctx_sync adds its time to the stats `blocks` selects
hipError_t timing_begin(fhh_ctx* ctx, size_t* slot);
hipError_t timing_end(fhh_ctx* ctx, size_t slot, uint64_t blocks);
// `blocks` tags of the event pairs that bracket the level loop's cross-rank all-reduce and its
// GC + OT step (share planes to the last chunk's sums)
constexpr uint64_t kAllreduceTag = ~0ull;
constexpr uint64_t kGcotTag = ~1ull;
// Pair mode (in-process two-server harness): c1 runs on c0's stream, so one stream carries
// both servers' work in order and the level loop needs a single host sync.
struct PairScope {
    fhh_ctx *c0, *c1;
    PairScope(fhh_ctx* a, fhh_ctx* b) : c0(a), c1(b) {
        c1->stream = c0->stream;
        c0->peer = c1;
    }
    ~PairScope() {
        (void)hipStreamSynchronize(c0->stream);
        c1->stream = c1->own_stream;
        c0->peer = nullptr;
    }
};
int crawl_pair(fhh_ctx* c0, fhh_ctx* c1, bool last);
ChildArgs child_args(fhh_ctx* c0, fhh_ctx* c1);   // ctx_child_args with server 1's tables from c1 (NULL: c0's)
int prune_impl(fhh_ctx* ctx, const uint8_t* keep, uint64_t n);
// FE255 values as arrays over field_arith.h's pointer forms: 8 u64 limb sums (limb k weight 2^(32k)) carry-propagated
// into 10 u32 limbs; their reduction mod p; a - b mod p
inline Limbs10 limbs_from_partials(const uint64_t* p8) {
    Limbs10 out{};
    fhh::limbs10_from_partials(p8, out.data());
    return out;
}
inline std::array<uint32_t, 8> fe255_reduce(const Limbs10& x) {
    std::array<uint32_t, 8> out{};
    fhh::fe255_reduce(x.data(), out.data());
    return out;
}
inline std::array<uint32_t, 8> fe255_sub(const std::array<uint32_t, 8>& a, const std::array<uint32_t, 8>& b) {
    std::array<uint32_t, 8> out{};
    fhh::fe255_sub(a.data(), b.data(), out.data());
    return out;
}
int alloc_keys(fhh_ctx* ctx, uint64_t n);   // the key buffers and `valid` of n clients (a one-shot layout)
int upload_staged(fhh_ctx* ctx);            // keys staged by fhh_add_keys to the device, as tree_init(_at) does
int finish_appended(fhh_ctx* ctx);          // fhh_keys_io.cpp: tree_init on appended keys
#pragma GCC visibility pop

// tree_crawl(_last)'s expansion; the share planes [C][2d][nw] (NULL: none) go to a host buffer
// whose rows are pitch_words u64 wide, this ctx's words starting at word_off (a shard of a
// multi-device ctx writes its 64-client words into the group's planes in place)
int crawl_level(fhh_ctx* ctx, bool last, uint64_t* n_children, uint64_t* planes, uint64_t pitch_words,
                uint64_t word_off);
// per-child 32-bit-limb partials of this ctx's OT outputs, enqueued on its stream (no sync):
// [C][2] (FE formats) or [C][8] (FE255); vals [C][ld] in format fmt, on the host (this ctx's
// clients at columns col0 .. col0 + n) or on the ctx's device (columns 0 .. n)
int node_partials(fhh_ctx* ctx, const void* vals, uint32_t fmt, uint64_t ld, uint64_t col0, bool host,
                  uint64_t** partials_dev);
// canonical FE sums [C] / unreduced [C][10] + canonical [C][8] FE255 sums from reduced partials;
// FE255 sums of a pending crawl_last become the frontier_last values (collect.rs:909-914)
int node_sums_finish(fhh_ctx* ctx, const uint64_t* partials, uint32_t fmt, void* out_a, void* out_b);
bool fmt_is_fe255(uint32_t fmt);

// fhh_frontier_plan's computation: a frontier given as paths [n_nodes][d][depth] (bytes 0/1) in the engine's
// per-dim, de-duplicated form, and its trie as `hist` holds a crawl's history
struct FrontierPlan {
    std::vector<uint32_t> n_unique;              // [d] distinct dim-j prefixes
    std::vector<uint32_t> pos;                   // [n_nodes][d] index of the node's dim-j prefix, first-appearance order
    std::vector<std::vector<uint64_t>> rep;      // [d][n_unique[j]] the first node that carries the prefix
    std::vector<std::vector<std::pair<uint32_t, uint32_t>>> hist;   // per depth: the distinct nodes as (parent, i)
};
// false (with the reason in *err) for the arguments fhh_tree_init_at refuses, data_len apart
bool frontier_plan(uint32_t d, uint32_t depth, uint64_t n_nodes, const uint8_t* paths, FrontierPlan& plan,
                   std::string* err);
// fhh_tree_init_at on a one-GPU ctx with the plan made (a multi-device ctx plans once for its shards)
int tree_init_at_planned(fhh_ctx* ctx, const FrontierPlan& plan, uint64_t n_nodes, uint32_t depth, const uint8_t* paths);

// ---- fhh_keys_io.cpp -------------------------------------------------------------------------
// the add_keys RPC payload's n client records (without the leading u64), decoded on the device
int add_keys_bincode_records(fhh_ctx* ctx, uint64_t n, const uint8_t* recs);
// fhh_reserve_clients / fhh_add_keys_bincode_append on a one-GPU ctx, in the steps a multi-device ctx drives
// per shard: the state check, the decode of m records onto the clients [n, n + m) (the layout grown first if
// need be; *herr = the kernels' malformed-field bits, the count not advanced), then commit (n += m) or
// rollback (the lanes from n on in n's word zero again, as before the batch)
int append_reserve(fhh_ctx* ctx, uint64_t capacity);
int append_check_state(fhh_ctx* ctx);
int append_decode(fhh_ctx* ctx, uint64_t m, const uint8_t* recs, uint32_t* herr);
void append_commit(fhh_ctx* ctx, uint64_t m);
int append_rollback(fhh_ctx* ctx);
std::string bincode_malformed_text(uint32_t herr);
// fhh_export_keys_bincode on one GPU, as a multi-device ctx drives it per shard: clients [src_first,
// src_first + m) of ctx's device keys are clients [i0, i0 + m) of an export of `count` clients in requests of B
// (bincode_emit.h); their bytes [be_slice_begin(i0), be_slice_end(i0, m)) are serialized on ctx's GPU and
// copied to the same offsets of `out`. Returns when they are there; the ctx is otherwise as before.
int export_bincode_check(fhh_ctx* ctx, bool have_keys, uint64_t n, uint64_t first, uint64_t count, uint64_t batch,
                         const uint8_t* out, uint64_t cap, uint64_t* len);   // the refusals; sets *len
int export_bincode_slice(fhh_ctx* ctx, uint64_t src_first, uint64_t m, uint64_t i0, uint64_t count, uint64_t B,
                         uint8_t* out);

// ---- fhh_retain.cpp --------------------------------------------------------------------------
// fhh_retain_plan's computation: false (with the reason in *err) for the masks it refuses
bool retain_plan(const uint8_t* keep, uint64_t n, std::vector<uint32_t>& src, std::string* err);
// The destination of one ctx's retain: everything the survivors' collection holds, built beside the ctx and
// swapped in by retain_commit, so that a failure (and a multi-device ctx whose other shard fails) leaves the
// ctx as it was.
struct RetainStage {
    uint64_t n2 = 0, nw2 = 0, npad2 = 0;
    bool device = false;          // the ctx's keys are on the device (else staged by fhh_add_keys: the h_* vectors)
    bool tables = false;          // frontier phase: every dim's live entries, made dense
    std::vector<uint8_t> h_key_idx, h_root, h_cws, h_cwb;
    DevBuf cw_seed, cw_bits, root_seed, key_idx, valid, lists;
    DevBuf seed[kMaxDims], t[kMaxDims], y[kMaxDims];
    size_t cap[kMaxDims] = {0, 0, 0, 0};
    double ms[2] = {0, 0};
    uint64_t bytes[2] = {0, 0};
    double emit_ms = -1;          // k_keep_emit's time when the list came from a device mask
};
// A keep mask in device memory (fhh_retain_clients_device): n_rows rows of n bytes, row r at keep + r * row_stride,
// resident on `device`; a client survives iff its byte is 1 in every row.
struct KeepMask {
    const uint8_t* keep = nullptr;
    uint64_t n = 0;
    uint32_t n_rows = 0;
    uint64_t row_stride = 0;
    int device = 0;
};
// what keep_scan_run leaves in ctx->keep_scan for the emit kernel (device pointers, valid until its next run)
struct KeepScan {
    const uint64_t* words = nullptr;
    const uint32_t* base = nullptr;
    uint64_t nw = 0;
};
// the argument refusals of the device-mask calls and the pointer check (no kernel, no ctx); fills m
bool keep_mask_check(const uint8_t* keep_dev, uint64_t n, uint32_t n_rows, uint64_t row_stride, KeepMask& m,
                     std::string* err);
// the AND of m's rows on the host, for keys that are staged there; FHH_E_ARG for a byte other than 0/1
int keep_mask_to_host(const KeepMask& m, std::vector<uint8_t>& keep, std::string* err);
// k_keep_words + k_keep_scan over clients [first, first + count) of m on ctx's device and stream (the rows copied
// there first if the mask lives elsewhere), the record read back; returns once the stream has drained
int keep_scan_run(fhh_ctx* ctx, const KeepMask& m, uint64_t first, uint64_t count, KeepScan& ks, KeepRecord& rec);
bool keep_record_check(const KeepRecord& rec, std::string* err);   // false for a bad byte or no survivor
int retain_check_state(fhh_ctx* ctx);   // FHH_E_STATE in the phases fhh_retain_clients refuses (one-GPU ctx)
// gather the n2 survivors of a one-GPU ctx into `st` (allocated before the first launch; returns once the stream
// has drained); the ctx is not changed. The survivor list is src[0 .. n2) on the host, or (src NULL) the one
// k_keep_emit writes from `scan`
int retain_prepare(fhh_ctx* ctx, const uint32_t* src, const KeepScan* scan, uint64_t n2, RetainStage& st);
void retain_commit(fhh_ctx* ctx, RetainStage& st);   // host only: cannot fail
// the survivors' records of add_keys-layout host vectors
void retain_host_keys(const fhh_ctx* ctx, const uint32_t* src, uint64_t n2, RetainStage& st);

// ---- fhh_join.cpp ----------------------------------------------------------------------------
// fhh_join_clients_bincode on a one-GPU ctx, in the steps a multi-device ctx drives for its last shard: the
// states it refuses, the request's framing (*m clients, their records from req + 8 on), and the join of m records
// (every refusal and failure leaves the ctx as it was)
int join_check_state(fhh_ctx* ctx);
// n + m clients are a count the engine holds: at most 2^32 - 2, so that every client index and the count itself
// stay below the u32 all-ones word
inline bool join_count_fits(uint64_t n, uint64_t m) { return !(n >> 32) && !(m >> 32) && n + m < 0xFFFFFFFFull; }
int join_parse(fhh_ctx* ctx, const uint8_t* req, uint64_t len, uint64_t* m);
int join_one(fhh_ctx* ctx, uint64_t m, const uint8_t* recs);

// ---- fhh_group.cpp (multi-device ctx) --------------------------------------------------------
int group_join_clients_bincode(fhh_ctx* g, const uint8_t* req, uint64_t len);
int group_retain_clients(fhh_ctx* g, const uint8_t* keep, uint64_t n);
int group_retain_clients_device(fhh_ctx* g, const uint8_t* keep_dev, uint64_t n, uint32_t n_rows, uint64_t row_stride,
                                uint64_t* n_kept);
fhh_ctx* group_shard0(const fhh_ctx* g);   // the first shard, whatever it holds (its device and stream)
void group_destroy(fhh_ctx* g);
int group_reset(fhh_ctx* g);
int group_set_client_base(fhh_ctx* g, uint64_t base);
int group_add_keys_bincode(fhh_ctx* g, const uint8_t* req, uint64_t len);
int group_reserve_clients(fhh_ctx* g, uint64_t capacity);
int group_add_keys_bincode_append(fhh_ctx* g, const uint8_t* req, uint64_t len);
bool group_appended(const fhh_ctx* g);
int group_gen_keys_pair(fhh_ctx* g0, fhh_ctx* g1, uint64_t n, const uint8_t* left, const uint8_t* right,
                        const uint8_t* roots);
int group_gen_keys_ball(fhh_ctx* g0, fhh_ctx* g1, uint64_t n, const fhh_ball_src* src);
// fhh_ball.cpp: fhh_gen_keys_ball on one-GPU ctxs (a carry out is named client_off + its index), and the refusals
// of a source for a collection of d dims and L levels
int gen_keys_ball_one(fhh_ctx* c0, fhh_ctx* c1, uint64_t n, const fhh_ball_src* src, uint64_t client_off);
bool ball_src_check(uint32_t d, uint32_t L, uint64_t n, const fhh_ball_src* src, std::string* why);
// fhh_ball.cpp: fhh_leader_requests_ball on one GPU, in the steps a multi-device ctx drives per shard: the m
// clients of `src` made on ctx's GPU as clients [i0, i0 + m) of an export of `count` clients in requests of B
// (returns when the kernel has run; a carry out is refused naming client i0 + its index), then their bytes
// copied to the same offsets of out0 / out1
int leader_requests_make(fhh_ctx* ctx, uint64_t m, const fhh_ball_src* src, uint64_t i0, uint64_t count, uint64_t B);
int leader_requests_copy(fhh_ctx* ctx, uint64_t m, uint64_t i0, uint64_t B, uint8_t* out0, uint8_t* out1);
int group_leader_requests_ball(fhh_ctx* g, uint64_t n, const fhh_ball_src* src, uint64_t batch, uint8_t* out0,
                               uint8_t* out1);
// fhh_ball.cpp: bytes of one (client, dim) point of a form, and the text of a carry out at index c d + j
size_t point_bytes(uint32_t form, uint32_t L);
std::string carry_text(uint64_t idx, uint32_t d, uint32_t L);
// fhh_audit.cpp: fhh_audit_keys_ball on one-GPU ctxs. The ok bytes stay in c0->audit_buf (audit_ok_dev) and go to
// ok_host where given; failures and a carry out are named client_off + their index.
struct AuditOut {
    uint64_t n_checks = 0, n_bad = 0, first = ~0ull, diverged = 0;   // first: AuditArgs' packed failure, global client
};
int audit_keys_one(fhh_ctx* c0, fhh_ctx* c1, uint64_t n, const fhh_ball_src* src, uint64_t client_off, uint8_t* ok_host,
                   AuditOut* out);
int audit_copy_ok(fhh_ctx* c0, uint64_t n, uint8_t* ok_host);   // the ok bytes of c0's last audit, to the host
int group_audit_keys_ball(fhh_ctx* g0, fhh_ctx* g1, uint64_t n, const fhh_ball_src* src, uint8_t* ok, AuditOut* out);
int group_num_clients(const fhh_ctx* g, uint64_t* n);
int group_export_keys(fhh_ctx* g, uint8_t* key_idx, uint8_t* root_seed, uint8_t* cw_seed, uint8_t* cw_bits);
int group_export_keys_bincode(fhh_ctx* g, uint64_t first, uint64_t count, uint64_t batch, uint8_t* out, uint64_t cap,
                              uint64_t* len);
int group_tree_init(fhh_ctx* g);
int group_tree_init_at(fhh_ctx* g, const FrontierPlan& plan, uint64_t n_nodes, uint32_t depth, const uint8_t* paths);
int group_tree_crawl(fhh_ctx* g, bool last, uint64_t* n_children, uint64_t* planes);
int group_node_sums(fhh_ctx* g, const void* const* vals, bool host, uint64_t ld, uint32_t fmt, void* out_a,
                    void* out_b);
int group_tree_prune(fhh_ctx* g, const uint8_t* keep, uint64_t n, bool last);
fhh_ctx* group_lead(const fhh_ctx* g);   // first shard with clients (frontier / final shares)
int group_export_states(fhh_ctx* g, uint64_t* n_nodes, uint8_t* seeds, uint8_t* t, uint8_t* y);
int group_sim_crawl(fhh_ctx* g0, fhh_ctx* g1, const fhh_sim_config* cfg);
int group_get_stats(const fhh_ctx* g, fhh_stats* out);
int group_each(fhh_ctx* g, int (*fn)(fhh_ctx*, int), int arg);   // set_variant / set_timing / reset_stats

void party_destroy(fhh_ctx* ctx);   // fhh_gcot.cpp

// ---- fhh_gcot.cpp (row f1) -------------------------------------------------------------------
void host_key_schedule(const uint8_t key[16], uint32_t (&rk)[11][4]);
// [3][128][44] key schedules of 128 base OTs: pairs [128][2][16] -> rows 0 / 1, chosen [128][16] -> row 2
// (a null source: its rows zero)
void base_ot_schedules(const uint8_t* pairs, const uint8_t* chosen, uint32_t* rk);
void words_from_bytes(const uint8_t b[16], uint32_t (&w)[4]);
uint64_t host_mix64(uint64_t z);
void gc_level_material(uint64_t prf_seed, uint32_t level, uint8_t key[16], uint8_t delta[16], uint32_t* mask);
void gc_chunk_material(uint64_t prf_seed, uint32_t level, uint64_t chunk, uint8_t key[16], uint8_t delta[16],
                       uint32_t* mask);
int gc_args(fhh_ctx* ctx, const fhh_gc_batch* b, GcArgs& a);
uint64_t ot_padded(uint64_t m);
void ot_level_choice(uint64_t prf, uint32_t level, uint32_t salt, uint32_t s[4]);
hipError_t ot_choices_buffer(fhh_ctx* ctx, uint64_t m, uint32_t** out);
struct OtOut {            // optional transcript (device pointers into the scratch)
    const uint4* U = nullptr;
    const uint4* Y0 = nullptr;
    const uint4* Y1 = nullptr;
    uint64_t nblk = 0;
    uint32_t u_rows = 128;            // 128 / ss_k (SoftSpoken)
    const uint4* corr = nullptr;      // SoftSpoken: the GGM corrections [u_rows][ss_k][2]
};
int ot_host_keys(fhh_ctx* ctx, const uint8_t seeds[128 * 2 * 16], const uint8_t s[16], const uint32_t** rk_dev);
// m OTs of OtArgs a's mode on ctx's stream (fhh_gcot.cpp): sizes, scratch matrices and messages are
// set here; tr (optional) receives the transcript's device pointers
int ot_run(fhh_ctx* ctx, OtArgs a, uint64_t m, OtOut* tr);
// the transcript's U in row form [u_rows][ceil(m / 128)][16], to the host
int u_transcript(fhh_ctx* ctx, const OtOut& tr, uint64_t m, uint8_t* u_out);
// row-PRG blocks a batch of m OTs takes from its base-OT session (a multiple of 256)
uint64_t ot_session_blocks(uint64_t m);

}  // namespace eng
}  // namespace fhh
