// Internal interface between the host engine (the .cpp sources, fhh_engine.h) and the HIP kernels
// (the .hip sources). Not part of the public C ABI (include/fhh.h).
//
// Device layout of one server's keys and evaluation states (SoA, lane = client):
//   npad = 64 * nw clients (padded), K = 2*d keys per client, kk = 2*j + side
//   cw_seed   [L][K][npad]   uint4      CorWord.seed            (ibDCF.rs:9-14)
//   cw_bits   [L][K][4][nw]  u64 planes bits.0, bits.1, y.0, y.1
//   root_seed [K][npad]      uint4      ibDCFKey.root_seed      (ibDCF.rs:16-21)
//   key_idx   [K][nw]        u64 plane  ibDCFKey.key_idx
//   per dim j, prefix table (double buffered), entry e = one dim-j prefix:
//     seed [E][2][npad] uint4, t [E][2][nw] u64, y [E][2][nw] u64   (EvalState, ibDCF.rs:24-30)
// A frontier node is a tuple of d entries (one per dim); a dim-j prefix shared by several
// nodes is evaluated once (the reference re-evaluates it per node, collect.rs:94-119).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "gt_plan.h"

struct fhh_comm;   // include/fhh.h (fhh_comm.cpp)

namespace fhh {

constexpr int kMaxDims = 4;
constexpr int kMaxJobs = 2 * kMaxDims;      // two servers' ctxs x dims in one launch
constexpr int kExpandThreads = 512;
constexpr int kReduceThreads = 256;

struct ExpandJob {
    const uint4* cw_seed;
    const uint64_t* cw_bits;
    const uint4* src_seed;
    const uint64_t* src_t;
    const uint64_t* src_y;
    uint4* dst_seed;
    uint64_t* dst_t;
    uint64_t* dst_y;
    const uint32_t* live;   // [n_live] src entries, in frontier order
    uint32_t n_live;
    uint32_t level;
    uint32_t dim;
    uint32_t K;
    uint32_t npad;
    uint32_t nw;
    uint32_t group;         // entries per work item (CW reuse factor)
    uint64_t item_begin;    // the launch's first item of this job
};

// Device-resident level loop (fhh_sim_crawl with the GPU loop): the frontier sizes live in
// device memory, written by k_prune and read by the next level's kernels, so a whole crawl is
// enqueued without host round trips. `abort` is sticky: once a capacity check fails every
// later kernel is a no-op and the host grows the buffers and resumes from abort_level.
struct LoopCtl {
    uint32_t abort;
    uint32_t abort_level;
    uint32_t need_entries;      // entries a dim table must hold to continue
    uint32_t need_nodes;        // frontier nodes to continue
    uint32_t F;                 // frontier nodes
    uint32_t C;                 // pending children (F << d)
    uint32_t n_live[kMaxDims];  // live entries per dim (same for both servers)
    uint32_t group;             // entries per work item for the next k_expand
    uint32_t wpi;               // words per item (item_layout)
    uint64_t item_begin[kMaxJobs];
    uint64_t total_items;
};

// k_expand work decomposition, shared by the host (finalize_launch) and the device loop
// (k_prune, k_loop_init). An item is g entries x wpi word units (64 clients each), g sized so
// each wave gets >= 2 items, capped at max_group (the CorWord reuse). Every item of a launch has
// the same shape: re-cutting the launch's last items smaller (against the wait for the slowest
// wave) measured no gain.
// Words per item (max_wpi > 1): when the frontier is narrow (d = 2 at data_len 16, or the first
// levels of any crawl) a group holds only a few entries, so one-word items are too small for the
// single counter — configs[3] at 1M clients made 62 500 items of ~2.5 entries per level and
// k_expand ran at the counter's 88 items/µs (25 G blocks/s). An item then spans
// wpi = max_group / (entries per group) consecutive words (64-client units), lowered until the
// launch still has kMwItemsPerWave items per wave; wide levels (groups of ≥ max_group / 2 entries)
// keep wpi = 1.
// r05: 4 (was 2) since k_expand draws from 8 per-XCD heads on narrow levels: configs[3] k_expand
// 0.44 -> 0.47 of the VALU roofline, the d = 1 headline unchanged (profiles/r05/expand_heads/)
// (r06 A/B, profiles/r06/ab_mw_ipw/: 2 -> 0.459, 8 or 16 -> 0.166 — wpi falls to 1 — against 0.478)
#ifndef FHH_MW_IPW
#define FHH_MW_IPW 4
#endif
constexpr uint64_t kMwItemsPerWave = FHH_MW_IPW;
struct ItemLayout {
    uint32_t g, wpi;
    uint64_t total;
    uint64_t begin[kMaxJobs];   // each job's first item
};
__host__ __device__ inline void item_layout(const uint32_t* n_live, uint32_t njobs, uint32_t unit, uint32_t max_group,
                                            uint64_t grid_waves, ItemLayout& L, uint32_t max_wpi = 1) {
    uint64_t entries = 0;
    for (uint32_t k = 0; k < njobs; k++) entries += n_live[k];
    const uint64_t entry_words = entries * unit;
    uint64_t g = entry_words / (2 * grid_waves);
    g = g < 1 ? 1 : (g > max_group ? max_group : g);
    L.g = (uint32_t)g;
    uint64_t wpi = 1;
    if (max_wpi > 1) {
        uint64_t groups = 0;
        for (uint32_t k = 0; k < njobs; k++) groups += (n_live[k] + g - 1) / g;
        if (groups) {
            const uint64_t e_eff = entries / groups;   // >= 1: every group holds an entry
            wpi = e_eff >= max_group ? 1 : max_group / e_eff;
            if (wpi > max_wpi) wpi = max_wpi;
            while (wpi > 1 && groups * ((unit + wpi - 1) / wpi) < kMwItemsPerWave * grid_waves) wpi--;
        }
    }
    L.wpi = (uint32_t)wpi;
    const uint64_t units = (unit + wpi - 1) / wpi;   // items per entry group
    uint64_t begin = 0;
    for (uint32_t k = 0; k < njobs; k++) {
        L.begin[k] = begin;
        begin += units * ((n_live[k] + g - 1) / g);
    }
    L.total = begin;
}

// One job's item `local` (= item - its begin) of a layout: entry group local / ceil(nw / wpi), words
// [w0, w1) of chunk local % ceil(nw / wpi), entries [e0, e1) (wpi = 1: group local / nw, word
// local % nw). k_expand decodes its items with this.
struct ItemRange {
    uint32_t w0, w1, e0, e1;
};
__host__ __device__ inline ItemRange item_range(uint64_t local, uint32_t n_live, uint32_t nw, uint32_t g, uint32_t wpi) {
    const uint32_t chunks = (nw + wpi - 1) / wpi;
    const uint32_t grp = (uint32_t)(local / chunks), w0 = (uint32_t)(local % chunks) * wpi;
    const uint32_t e0 = grp * g;
    ItemRange r;
    r.w0 = w0;
    r.w1 = w0 + wpi < nw ? w0 + wpi : nw;
    r.e0 = e0;
    r.e1 = e0 + g < n_live ? e0 + g : n_live;
    return r;
}

// k_expand's dynamic work heads inside fhh_ctx::work_counter (kWorkCounterBytes): two sets of
// kExpandHeads per-XCD heads (one 64-B line each) by launch parity (the kernel zeroes the next
// launch's set), from word kExpandSlot0 on; the words before and after them are unused
constexpr uint32_t kExpandHeads = 8, kExpandSlot0 = 16, kExpandSlotStride = 16;
constexpr size_t kWorkCounterBytes = 2048;
static_assert((kExpandSlot0 + 2 * kExpandHeads * kExpandSlotStride) * 4 <= kWorkCounterBytes, "work counter layout");

struct ExpandLaunch {
    ExpandJob job[kMaxJobs];
    uint32_t njobs;
    uint32_t jobs_per_ctx;      // = d (LoopCtl::n_live index = job % jobs_per_ctx)
    uint64_t total_items;
    uint32_t wpi;               // host-driven launches: words per item (item_layout)
    uint32_t seq;               // the counter's launch number (fhh_ctx::expand_seq): k_expand counter slot
    const LoopCtl* ctl;         // non-null: n_live / group / item_begin / total_items from here
};

// Pending children: child c -> parent p = c >> d, i = c & (2^d - 1); its dim-j entry in
// the child table is 2 * parent_pos[p*d + j] + ((i >> j) & 1).
struct PlaneSet {
    const uint64_t* t[kMaxDims];
    const uint64_t* y[kMaxDims];
};

struct ChildArgs {
    PlaneSet s0, s1;            // server 0 / server 1 child tables (s1 unused for share export)
    const uint32_t* parent_pos; // [F][d]
    const uint64_t* valid;      // [nw]
    uint64_t C;
    uint32_t d;
    uint32_t nw;
    uint64_t client_base;       // global index of client 0 (simulated-OT PRF)
    uint64_t prf_seed;
    uint32_t level;
    uint32_t n;                 // real clients on this ctx
    const LoopCtl* ctl;         // non-null: C from here (0 once aborted)
    // GC mode (row f1): the equality bit of (child c, client i) is the evaluator's garbled-
    // circuit output gc_out[c * gc_N + i] XOR the garbler's mask (ideal OT, collect.rs:437-471)
    const uint8_t* gc_out;
    uint32_t gc_N;
    uint32_t gc_mask;
    // OT mode (r05: correlated OT, OtArgs modes 2 / 3): the two servers' node values of (c, i) are
    // the C-OT's outputs — FE levels u64 ot_val[s][(c - c_off) * gc_N + i] (s = 0 the garbler's
    // v + mask, s = 1 the receiver's); the last level BlockPairs (2 blocks per value: the garbler's
    // canonical V + mask, the receiver's raw FieldElm::try_from(BlockPair))
    const void* ot_val[2];
    // child window of the GC + OT kernels (a chunk of the level's children, as the reference splits
    // a level's tests over its channels, collect.rs:423-430): children [c_off, c_off + c_cnt) only,
    // gc_out / ot_recv / OT messages indexed (c - c_off) * gc_N + i; c_cnt = 0: every child
    uint64_t c_off;
    uint64_t c_cnt;
    // k_share_planes' row stride in words (0: nw); words nw .. plane_nw - 1 are written as zero (r06: the
    // tile-major garbled table wants rows of whole 512-client tiles, plane_nw a multiple of 8)
    uint32_t plane_nw;
};

// Garbled-circuit equality tests (row f1, equalitytest.rs:25-219): tests t = g * N + i for
// groups g < G (children) and i < N (clients); a test compares the garbler's `bits`-bit string
// with the evaluator's. Inputs are bit planes [G][bits][nw] (as k_share_planes writes them);
// outputs are SoA over t (16-B blocks; one lane per test, coalesced).
constexpr int kGcMaxBits = 8;
struct GcArgs {
    const uint64_t* gb_planes;   // garbler's share bits
    const uint64_t* ev_planes;   // evaluator's share bits (ideal OT: only their labels leave)
    uint64_t G;
    uint32_t N, nw, bits, mask;
    uint32_t rk_label[11][4];    // garbler's label PRG key schedule (AES-128-CTR)
    uint32_t delta[4];           // free-XOR offset, lsb 1
    uint64_t label_nonce;        // label of (t, w) = AES_k(label_nonce + t S + w), S = pow2 >= W (W = 2 bits + 1, ev_ot: bits + 1)
    uint64_t gate_base;          // half-gate tweaks 2 (gate_base + t (bits - 1) + k) (+1)
    uint4* tables;               // [(bits-1)][2][n]  (T_G, T_E)
    uint4* gb_labels;            // [bits + 1][n]     garbler's active input labels (+ mask)
    uint4* ev_labels;            // [bits][n]         evaluator's active labels (ideal OT out)
    uint8_t* decode;             // [n]               output decoding bit
    uint8_t* out;                // [n]               evaluator's output bit = eq ^ mask
    const LoopCtl* ctl;          // non-null (level loop): groups = min(G, ctl->C), 0 once aborted;
                                 // G * N stays the SoA stride
    uint32_t ev_ot;              // 1 (r05, the labels OT is a correlated OT): ev_labels holds the
                                 // evaluator's labels at OT index (g bits + j) Npad + i (Npad = 64 nw:
                                 // its share planes are the OT's choice bits) — k_gc_garble reads the
                                 // ZERO labels there (the C-OT's sender messages) and draws only its
                                 // own wires and the mask (label stride pow2 >= bits + 1), k_gc_eval
                                 // reads its OT'd active labels there. 0: ideal OT (every label drawn
                                 // by the garbler, the evaluator's active ones written to ev_labels)
    uint32_t out_dup;            // out_packed: each output bit repeated out_dup (1 or 2) times
    uint32_t* out_packed;        // non-null: k_gc_eval also writes the outputs as bit words
                                 // (tests t0.. of a 64-aligned wave slice; the FE-share OT choices)
    uint64_t g_off;              // chunk: groups [g_off, g_off + G) of the planes; tests, labels and
                                 // gate tweaks keep their whole-level index (g_off N + t)
    // r05c (ev_ot, FE levels): the FE share from the output labels instead of a second OT, [G N] each
    // (oracle gc_share_garbler / gc_share_evaluator): k_gc_garble_cot writes the garbler's node value
    // r1 = v + mask to sh_gb and the 8-B message y to sh_y; k_gc_eval reads sh_y and writes the
    // evaluator's node value to sh_ev. Null: no share.
    uint64_t* sh_gb;
    uint64_t* sh_y;
    uint64_t* sh_ev;
    // r05d (FE levels, bits <= kGtMaxBits): the garbled table (oracle orc_gt_garble / orc_gt_eval):
    // the garbler (k_gt_garble<B, RING> on row-major labels, bits = 3, 4; k_gt_garble_tm on tile-major ones)
    // writes rows 1 .. 2^bits - 1's messages SoA [2^bits - 1][G N] and its node values to sh_gb, the evaluator
    // (k_gt_eval<B, RING> / k_gt_eval_tm) reads them and writes its own to sh_ev
    uint64_t* gt_msgs;
    // r06: 1 = ev_labels is the labels OT's tile-major matrix itself (Q for k_gt_garble_tm, T for k_gt_eval_tm;
    // fhh_ot.hip ot_tmaj) instead of one row-major label per OT (k_ot_rows_out). bits <= kGtTmPadBits needs
    // nw % 8 == 0 (the OT index (g bits + k) 64 nw + i puts a test's labels at one position of 512-OT tiles);
    // bits = 3, 4 take any nw (a bit's 512-test window starts at any even word of a tile)
    uint32_t lab_tm;
    // r06 (lab_tm): non-null = the table kernels add their node values' 32-bit limbs per child into
    // node_partials [C][4] u64 (k_child_sums_fe's layout: garbler lo, hi; evaluator lo, hi) by one wave sum
    // and atomic per 512-test tile, instead of storing them for k_child_sums_fe (sh_gb / sh_ev may be null)
    uint64_t* node_partials;
    uint64_t node_off;   // node_partials row of the launch's group 0 beyond g_off (the party ABI: its chunk's c_off)
    // r06 (lab_tm): 1 = the table's shares live in Z_2^32 instead of FE (row value lo32 of the
    // hash, pair (v, v +- 1 mod 2^32), 4-B messages [2^b - 1][n] u32; the partials' low sums taken mod 2^32).
    // Without lab_tm (bits = 3, 4: k_gt_garble<B, true> / k_gt_eval<B, true>) sh_gb / sh_ev hold u32 values [G N] too
    uint32_t ring32;
};
// (kGtMaxBits, kGtTmMaxBits, kGtTmPadBits: gt_plan.h)

struct PruneArgs {
    LoopCtl* ctl;
    const uint64_t* partials;   // [C][per] u64 (after the cross-rank sum)
    uint32_t mode;              // 0 counts, 1 FE limbs [C][4], 2 FE255 limbs [C][16] (last level)
    uint32_t d;
    uint64_t thr;               // leader.rs:193-194
    uint32_t thr_last;          // leader.rs:245-246
    uint32_t last;              // tree_crawl_last: record final values
    const uint32_t* pos_in;     // [F][d]
    uint32_t* pos_out;          // [F'][d]
    uint32_t* live_out[kMaxDims];
    uint32_t* mark;             // scratch [kMaxDims][E_cap]
    uint32_t* hist_out;         // [F_cap] kept children of this level (child index c)
    uint32_t* sizes_out;        // [4 + kMaxDims]: C, F', abort, -, n_live'...
    uint32_t* final_vals;       // last level: [F_cap][20] u32 (server 0 / server 1 unreduced)
    uint32_t E_cap, F_cap;
    uint32_t level;
    uint32_t nw;
    uint32_t njobs_per_ctx;     // = d
    uint32_t nctx;              // 2 (pair)
    uint64_t grid_waves;        // persistent k_expand waves (for the group size)
    uint32_t unit;              // k_expand items per entry group (nw)
    uint32_t max_group;         // entries per item cap
    uint32_t max_wpi;           // item_layout words-per-item cap (expand_max_wpi)
    // FE levels: k_child_sums_fe adds its client chunks into the partials by atomics, so a prune that
    // completes zeroes them for the next level (a memset node would also run after a sticky
    // abort and wipe the sums the resumed prune re-reads)
    uint64_t* zero_partials;
    uint64_t zero_count;
    uint32_t ring32;            // r06, mode 1: the level's shares are in Z_2^32 (GcArgs::ring32): v0 - v1 mod 2^32
};

// k_keygen's sources of a key's bits (launch_keygen's `src`)
constexpr int kKeygenBytes = 0;      // left_bits / right_bits, a byte per bit (fhh_gen_keys_pair)
constexpr int kKeygenBallBits = 1;   // points: packed L-bit strings, the bounds a -/+ ball made in the kernel
constexpr int kKeygenCoords = 2;     // points: i16 (lat, long), the clamped bounds made in the kernel (d = 2, L = 16)
struct KeygenArgs {
    const uint8_t* left_bits;   // [n][d][L]
    const uint8_t* right_bits;
    const uint8_t* root_seeds;  // [n][d][2 side][2 server][16]; the point forms: NULL = drawn from `seed`
    uint4* cw_seed[2];
    uint64_t* cw_bits[2];
    uint4* root[2];
    uint64_t* key_idx[2];
    uint64_t n;
    uint32_t d, L, K, npad, nw;
    // the point forms (fhh_gen_keys_ball, ball_src.h)
    uint32_t ball;
    const uint8_t* points;      // kKeygenBallBits: [n][d][ceil(L / 8)]; kKeygenCoords: int16 [n][2]
    unsigned long long* bad;    // lowest c d + j whose right bound carries out of bit L (preset to ~0)
    uint32_t seed[8];           // ChaCha20 key of the derived root seeds
    uint64_t seed_first;        // global index of client 0 in the seed stream
};

// k_eval_paths (fhh_tree_init_at): every client's keys walked from the root to given prefixes. Job j = dim j's
// distinct prefixes, written as entries 0 .. n_prefixes - 1 of the dim's table; an item is one word (64
// clients) of one side of kEvalPathsP prefixes: job j has 2 nw ceil(n_prefixes / kEvalPathsP) items.
constexpr int kEvalPathsP = 4;
struct EvalPathsJob {
    uint4* dst_seed;            // [n_prefixes][2][npad]
    uint64_t* dst_t;            // [n_prefixes][2][nw]
    uint64_t* dst_y;
    const uint32_t* dirs;       // [n_prefixes][dir_words]: direction of level l = bit l % 32 of word l / 32
    uint32_t n_prefixes;
    uint64_t item_begin;        // the launch's first item of this job
};
struct EvalPathsArgs {
    const uint4* cw_seed;
    const uint64_t* cw_bits;
    const uint4* root_seed;
    const uint64_t* key_idx;
    EvalPathsJob job[kMaxDims];
    uint32_t d, K, npad, nw;
    uint32_t depth;             // levels walked (< L)
    uint32_t dir_words;         // ceil(depth / 32)
    uint64_t total_items;
};

// k_join_paths (fhh_join_clients_bincode): k_eval_paths' walk on the words [w_first, w_first + words) of the layout
// only — the clients that joined a ctx with a frontier. Job j's prefix e is the dim's e-th live entry and goes to
// table entry rows[j][e]; an item is one of those words of one side of kEvalPathsP prefixes (job j has
// 2 words ceil(n_prefixes / kEvalPathsP) items). In word w_first only the lanes of first_mask are written: the
// others hold the states of clients that were there before.
struct JoinPathsExtra {
    const uint32_t* rows[kMaxDims];   // [n_prefixes] table entry of each prefix
    uint64_t first_mask;              // lanes >= n % 64 (all ones when n % 64 == 0)
    uint32_t w_first;                 // n / 64
    uint32_t words;                   // new nw - w_first
};
// The launch of k_join_paths (fhh_join_plan): n clients held, m joining, U[j] live entries of dim j, at most
// grid_blocks workgroups of kAuditBlock (= k_eval_paths' 1024) threads
struct JoinPlan {
    uint64_t first_word, first_mask, words, new_nw, items, blocks, waves, trips, last_trip_items, aes_blocks;
};
__host__ __device__ inline JoinPlan join_plan(uint32_t d, uint32_t depth, uint64_t n, uint64_t m, const uint32_t* U,
                                              uint64_t grid_blocks) {
    const uint64_t wpb = 1024 / 64;
    JoinPlan p;
    p.first_word = n / 64;
    p.first_mask = ~((n % 64) ? (1ull << (n % 64)) - 1 : 0ull);
    p.new_nw = (n + m + 63) / 64;
    p.words = p.new_nw - p.first_word;
    p.items = 0;
    uint64_t entries = 0;
    for (uint32_t j = 0; j < d; j++) {
        p.items += 2 * p.words * (((uint64_t)U[j] + kEvalPathsP - 1) / kEvalPathsP);
        entries += U[j];
    }
    p.blocks = (p.items + wpb - 1) / wpb;
    if (p.blocks > grid_blocks) p.blocks = grid_blocks;
    p.waves = p.blocks * wpb;
    p.trips = p.waves ? (p.items + p.waves - 1) / p.waves : 0;
    p.last_trip_items = p.trips ? p.items - (p.trips - 1) * p.waves : 0;
    p.aes_blocks = (uint64_t)depth * 2 * entries * m;
    return p;
}

// ---- launch wrappers (fhh_kernels.hip); all asynchronous on `stream` ----
// grid: at most this many workgroups (the persistent k_expand grid; the items are dealt grid-stride)
hipError_t launch_eval_paths(const EvalPathsArgs& a, int grid, hipStream_t stream);
// a.job[j].dst_* = the dim's current table at a.npad / a.nw, n_prefixes its live entries, dirs their directions;
// a.total_items / item_begin by JoinPathsExtra's item count
hipError_t launch_join_paths(const EvalPathsArgs& a, const JoinPathsExtra& x, int grid, hipStream_t stream);
// seq: the counter's launch count (fhh_ctx::expand_seq), advanced per k_expand launch
hipError_t launch_expand(const ExpandLaunch& a, int variant, int grid, uint32_t* work_counter, uint32_t* seq,
                         hipStream_t stream);
int expand_variant_count();
const char* expand_variant_name(int variant);
int expand_threads(int variant);
// item_layout's caps for the variant: entries per item, words per item (1: one-word items only)
uint32_t expand_max_group(int variant);
uint32_t expand_max_wpi(int variant);
hipError_t launch_eq_count(const ChildArgs& a, uint64_t* counts, hipStream_t stream);
hipError_t launch_share_planes(const ChildArgs& a, uint64_t* out, hipStream_t stream);
// zero: clear partials first (host-driven launches); the device loop's k_prune clears them instead
hipError_t launch_child_sums_fe(const ChildArgs& a, uint64_t* partials /*[C][4]*/, hipStream_t stream, bool zero);
hipError_t launch_child_sums_fe255(const ChildArgs& a, uint64_t* partials /*[C][16]*/, hipStream_t stream);
// per-child limb partials of values [C][ld] (n per row) in format fmt (FHH_VALS_*): FE -> [C][2],
// FE255 -> [C][8]
hipError_t launch_sum_vals(const void* vals, uint32_t fmt, uint64_t C, uint64_t n, uint64_t ld, uint64_t* partials,
                           hipStream_t stream);
hipError_t launch_keygen(const KeygenArgs& a, int src, hipStream_t stream);
hipError_t launch_init_tables(const uint4* root, const uint64_t* key_idx, uint32_t dim, uint32_t K, uint32_t npad,
                              uint32_t nw, uint4* seed, uint64_t* t, uint64_t* y, hipStream_t stream);
hipError_t launch_keys_from_aos(const uint8_t* key_idx, const uint8_t* root_seed, const uint8_t* cw_seed,
                                const uint8_t* cw_bits, uint64_t n, uint32_t K, uint32_t L, uint32_t npad, uint32_t nw,
                                uint4* d_cw_seed, uint64_t* d_cw_bits, uint4* d_root, uint64_t* d_key_idx,
                                hipStream_t stream);
hipError_t launch_keys_from_bincode(const uint8_t* buf, uint64_t n, uint32_t d, uint32_t L, uint32_t npad, uint32_t nw,
                                    uint4* d_cw_seed, uint64_t* d_cw_bits, uint4* d_root, uint64_t* d_key_idx,
                                    uint32_t* err, hipStream_t stream);
// an appended batch: the m records of buf onto the clients [c0, c0 + m) of a layout of nw >= ceil((c0 + m) / 64)
// words (bincode_span.h); m = 0 re-zeroes the lanes from c0 on in c0's word
hipError_t launch_keys_from_bincode_at(const uint8_t* buf, uint64_t c0, uint64_t m, uint32_t d, uint32_t L,
                                       uint32_t npad, uint32_t nw, uint4* d_cw_seed, uint64_t* d_cw_bits, uint4* d_root,
                                       uint64_t* d_key_idx, uint32_t* err, hipStream_t stream);
// `rows` rows of `width` elements from row pitch src_pitch to dst_pitch (elements): a change of the key
// layout's capacity
hipError_t launch_repitch_seeds(const uint4* src, uint4* dst, uint64_t rows, uint64_t width, uint64_t src_pitch,
                                uint64_t dst_pitch, hipStream_t stream);
hipError_t launch_repitch_words(const uint64_t* src, uint64_t* dst, uint64_t rows, uint64_t width, uint64_t src_pitch,
                                uint64_t dst_pitch, hipStream_t stream);
// fhh_retain.hip (fhh_retain_clients): n_rows rows of the survivors idx[0 .. n2) (old client indices, increasing)
// from row pitch npad / nw into a buffer of pitch npad2 / nw2, zero beyond n2; rows (may be null) = the source
// row of each destination row. src and dst never overlap.
hipError_t launch_retain_cols(const uint4* src, uint4* dst, const uint32_t* idx, const uint32_t* rows, uint64_t n_rows,
                              uint64_t npad, uint64_t npad2, uint32_t n2, hipStream_t stream);
hipError_t launch_retain_planes(const uint64_t* src, uint64_t* dst, const uint32_t* idx, const uint32_t* rows,
                                uint64_t n_rows, uint64_t nw, uint64_t nw2, uint32_t n2, hipStream_t stream);
// fhh_retain_mask.hip (fhh_retain_clients_device): that idx list from a keep mask in device memory, n_rows rows of
// n < 2^32 bytes at keep + r * row_stride, a client kept iff its byte is 1 in every row. launch_keep_scan leaves
// the keep words [nw], their exclusive prefix counts base [nw] (nw = ceil(n / 64)) and the record;
// launch_keep_emit writes idx[0 .. n_kept) from them.
struct KeepRecord {
    uint64_t n_kept;   // survivors
    uint64_t bad;      // (client index << 8 | byte) of the lowest client with a byte other than 0/1; ~0: none
};
constexpr uint64_t kKeepNoBad = ~0ull;
hipError_t launch_keep_scan(const uint8_t* keep, uint64_t n, uint32_t n_rows, uint64_t row_stride, uint64_t* words,
                            uint32_t* base, KeepRecord* rec, hipStream_t stream);
hipError_t launch_keep_emit(const uint64_t* words, const uint32_t* base, uint64_t nw, uint32_t* idx,
                            hipStream_t stream);
// fhh_bincode_out.hip: clients [src_first, src_first + m) of the layout as clients [i0, i0 + m) of an export of
// `count` clients in requests of B (bincode_emit.h); byte g of the export goes to stg[g - org], org % 4 == 0 and
// org <= be_slice_begin(i0), stg holding be_slice_end(i0, m) - org bytes
hipError_t launch_bincode_emit(const uint4* cw_seed, const uint64_t* cw_bits, const uint4* root_seed,
                               const uint64_t* key_idx, uint32_t d, uint32_t L, uint32_t npad, uint32_t nw,
                               uint64_t src_first, uint64_t m, uint64_t i0, uint64_t count, uint64_t B, uint8_t* stg,
                               uint64_t org, hipStream_t stream);
// fhh_leader_requests.hip (fhh_leader_requests_ball): k_keygen's point forms with the serialization fused in. The n
// clients of `points` are clients [i0, i0 + n) of an export of `count` clients in requests of B (bincode_emit.h);
// byte g of server b's requests goes to out[b][g - org], org % 4 == 0, org <= be_slice_begin(i0), out[b] dword
// aligned and holding be_slice_end(i0, n) - org bytes. No key buffer is read or written.
struct LeaderReqArgs {
    const uint8_t* points;      // as KeygenArgs: kKeygenBallBits [n][d][ceil(L / 8)]; kKeygenCoords int16 [n][2]
    const uint8_t* root_seeds;  // [n][d][2 side][2 server][16], or NULL = drawn from `seed`
    unsigned long long* bad;    // lowest c d + j whose right bound carries out of bit L (preset to ~0)
    uint8_t* out[2];
    uint64_t org;
    uint64_t n, i0, count, B;
    uint32_t d, L, ball;
    uint32_t seed[8];
    uint64_t seed_first;        // global index of client 0 of `points` in the seed stream
};
// The launch of k_leader_requests (fhh_leader_requests_plan): an item is one wave's 64 clients of one key, as
// k_keygen's; the items are dealt grid-stride to at most kLeaderReqMaxBlocks workgroups of kExpandThreads
constexpr uint64_t kLeaderReqMaxBlocks = 4096;
struct LeaderReqPlan {
    uint64_t items, waves, trips;
};
__host__ __device__ inline LeaderReqPlan leader_req_plan(uint32_t d, uint64_t n) {
    const uint64_t wpb = kExpandThreads / 64;
    LeaderReqPlan p;
    p.items = 2ull * d * ((n + 63) / 64);
    uint64_t blocks = (p.items + wpb - 1) / wpb;
    if (blocks > kLeaderReqMaxBlocks) blocks = kLeaderReqMaxBlocks;
    p.waves = blocks * wpb;
    p.trips = p.waves ? (p.items + p.waves - 1) / p.waves : 0;
    return p;
}
hipError_t launch_leader_requests(const LeaderReqArgs& a, int src, hipStream_t stream);
// fhh_audit.hip (fhh_audit_keys_ball, row j): both servers' keys of every client evaluated at the five probes of
// its point (ball_src.h) and every prefix's reconstructed bit compared with the interval rule. An item is one
// wave's 64 clients of one key (dim j, side), lane = client; it walks the 5 probes with both servers' keys, 10
// AES blocks per level. Each server's keys come in their own layout (an appended collection keeps its capacity
// stride until tree_init).
struct AuditSrv {
    const uint4* cw_seed;
    const uint64_t* cw_bits;
    const uint4* root_seed;
    const uint64_t* key_idx;
    uint32_t npad, nw;
};
// a failure as one u64, ordered as (client, dim, side, probe, level): client << 25 | dim << 23 | side << 22 |
// probe << 19 | level << 1 | expected bit (level = 1 .. L < 2^18: the prefix length compared)
constexpr uint32_t kAuditMaxLevels = (1u << 18) - 1;
constexpr uint32_t kAuditRecWords = 5;
struct AuditArgs {
    AuditSrv srv[2];
    const uint8_t* points;      // as KeygenArgs: kKeygenBallBits [n][d][ceil(L / 8)]; kKeygenCoords int16 [n][2]
    uint8_t* ok;                // [n], preset to 1: cleared for a client with a failed comparison
    // [0] the lowest failure (preset to ~0), [1] comparisons made (0), [2] lowest c d + j whose right bound carries
    // out of bit L (~0), [3] clients with ok = 0 (0; k_audit_count), [4] walks that end off the key's path with the
    // two servers' seeds unequal (0)
    unsigned long long* rec;
    uint64_t n;
    uint32_t d, L, K, ball;
};
// The launch of k_audit_keys (fhh_audit_plan): k_eval_paths' shape, workgroups of kAuditBlock threads, at most
// `grid_blocks` of them, the items dealt grid-stride
constexpr int kAuditBlock = 1024;
struct AuditPlan {
    uint64_t items, blocks, waves, trips, last_trip_items, aes_blocks, n_checks;
};
__host__ __device__ inline AuditPlan audit_plan(uint32_t d, uint32_t L, uint64_t n, uint64_t grid_blocks) {
    const uint64_t wpb = kAuditBlock / 64;
    AuditPlan p;
    p.items = 2ull * d * ((n + 63) / 64);
    p.blocks = (p.items + wpb - 1) / wpb;
    if (p.blocks > grid_blocks) p.blocks = grid_blocks;
    p.waves = p.blocks * wpb;
    p.trips = p.waves ? (p.items + p.waves - 1) / p.waves : 0;
    p.last_trip_items = p.trips ? p.items - (p.trips - 1) * p.waves : 0;
    p.n_checks = n * 2 * d * 5 * L;
    p.aes_blocks = 2 * p.n_checks;   // both servers' keys at every (probe, level)
    return p;
}
// form: kKeygenBallBits / kKeygenCoords; also counts the cleared ok bytes into rec[3]
hipError_t launch_audit_keys(const AuditArgs& a, int form, int grid_blocks, hipStream_t stream);
// occupancy-derived persistent grid for k_expand variant on `device`
int expand_grid(int device, int variant);
// RCCL all-reduce (sum, u64) on `stream` (fhh_comm.cpp); asynchronous
int comm_allreduce(::fhh_comm* c, const uint64_t* send, uint64_t* recv, uint64_t count, hipStream_t stream,
                   std::string* err);
// in-process communicators over distinct devices (ncclCommInitAll), a grouped in-place all-reduce
// (ncclGroupStart/End, one stream per communicator) and abort (fhh_comm.cpp)
int comm_init_all(int n, const int* devices, std::vector<::fhh_comm*>& out, std::string* err);
int comm_group_allreduce(const std::vector<::fhh_comm*>& comms, const std::vector<uint64_t*>& bufs, uint64_t count,
                         const std::vector<hipStream_t>& streams, std::string* err);
// abort once (a second call, or one racing it from another shard thread, is a no-op); the handle
// stays valid until fhh_comm_destroy, which then skips ncclCommDestroy
void comm_abort(::fhh_comm* c);
int comm_rank(const ::fhh_comm* c);   // the rank given at creation
// device-resident level loop (fhh_loop.hip); `unit` = items per entry group, `max_group` =
// entries per item cap (expand_max_group)
hipError_t launch_prune(const PruneArgs& a, hipStream_t stream);
// IKNP / ALSZ OT extension (row f1's OT): m OTs of 16-B messages; base OTs given as key schedules
// (the sender's are those of k_i^{s_i}). Bit matrices are [128 rows][mp / 128] uint4 blocks, read per
// OT by the hashes (transposed on the fly). With ctl set (level loop) only the first
// per_group * min(groups, ctl->C) OTs run.
// Modes (r05; oracle/fhh_oracle.c orc_ot_extend / orc_cot_extend):
//   0  plain OT: y_j^b = x_j^b ^ H(q_j ^ b s) (x1 == nullptr: x1 = x0 ^ delta); out = y_j^{r_j} ^ H(t_j)
//   1  correlated OT, XOR delta (the labels OT): sender writes sx[j] = H(q_j) (the evaluator's zero
//      label) and Y0[j] = H(q_j) ^ delta ^ H(q_j ^ s); out = r_j ? Y0[j] ^ H(t_j) : H(t_j)
//   2  correlated OT, FE share: v = H(q_j) as LE u128 mod p; sender value v + mask -> sx (u64 [m]),
//      Y0 (8 B [m]) = lo64(H(q_j ^ s)) ^ (mask ? v + 1 : v - 1); out (u64 [m]) = r_j ? lo64(Y0[j] ^
//      H(t_j)) : H(t_j) mod p
//   3  correlated OT, FieldElm share, raw pass: sx[j] = H(q_j), Y0[j] = H(q_j ^ s); k_cot_fe255_finish
//      turns OT pairs (2t, 2t + 1) into the sender's node values and y; out = r_j ? Y0[j] ^ H(t_j) : H(t_j)
//   4  (r05b) the IKNP correlation itself, the labels OT: no hash, no y — sx[j] = q_j, out[j] = t_j =
//      q_j ^ r_j s (k_ot_rows_out transposes Q / T); with s as the free-XOR Delta, q_j is the zero label
//      of the evaluator's input wire j and t_j its active label
struct OtArgs {
    uint64_t m;                  // OTs (capacity)
    uint64_t mp;                 // m padded to a multiple of 8192 (whole waves per row)
    const uint32_t* rk;          // [3][128][44]: receiver k_i^0, k_i^1, sender k_i^{s_i}
    uint32_t s[4];               // sender's base choice bits
    const uint32_t* choices;     // [mp / 32] receiver's choice bits (0 past m)
    uint4 *T, *U, *Q;            // tile-major (fhh_ot.hip ot_tmaj): T, Q, and since r06 U (the wire) too
    const uint4 *x0, *x1;        // mode 0: [m]; x1 == nullptr: x1 = x0 ^ delta (correlated messages)
    uint32_t delta[4];           // modes 0 (x1 == nullptr) and 1
    uint4 *Y0, *Y1, *out;        // mode 0: Y0, Y1 [m]; modes 1-3: y in Y0 (mode 2: 8 B per OT); out [m]
    uint64_t tweak_base;
    const LoopCtl* ctl;
    uint64_t per_group;
    uint64_t g_off;              // level loop chunk: OTs of groups [g_off, ctl->C) only
    uint32_t mode;               // 0..4 above; 5 = 4 left tile-major (expands only: the r06 garbled table
                                 // reads Q / T itself, GcArgs::lab_tm)
    uint32_t mask;               // modes 2, 3: the garbler's mask bit
    uint64_t ctr_off;            // the row PRG's first block (a multiple of 256): a base-OT session's
                                 // running counter, so batches extending one session never repeat pads
    void* sx;                    // modes 1, 3, 4: uint4 [m]; mode 2: u64 [m] (the sender's node values)
    // r06: 0 / 1 = IKNP; 2, 4 = SoftSpoken with k = ss_k (fhh_ot.hip k_ss_*): U is then 128 / k rows
    // (tile-major, tile stride 128 / k rows), ss_leaf [2][128 / k][2^k] the GGM leaves (receiver, sender),
    // ss_corr [128 / k][k][2] the receiver's GGM corrections (the wire)
    uint32_t ss_k;
    uint32_t ss_role;            // k_ss_ggm: 0 both parties (the level loop), 1 the receiver (leaves + corrections),
                                 // 2 the sender (its leaves from ss_corr, the received corrections) — the party ABI
    uint4* ss_leaf;
    uint4* ss_corr;
};
// ---- the launch grid of the GC / OT kernels whose workgroups stride over their work -------------------------
// CU count of the current device, queried once per device (fhh_ot.hip; 256 where the query fails)
int device_cus();
// the launcher families (fhh_protocol_grid's `family`) and the workgroups each may keep per CU
enum ProtocolGridFamily {
    kGridOtExpand = 0,    // k_ot_*_expand_cc, k_ss_*_expand: 256 threads, 20 KiB of LDS
    kGridOtHash = 1,      // k_ot_send_hash_rows, k_ot_recv_hash_rows: one 160-KiB workgroup per CU
    kGridOtRowsOut = 2,   // k_ot_rows_out
    kGridCotFinish = 3,   // k_cot_fe255_finish
    kGridGc = 4,          // k_gc_garble, k_gc_garble_cot, k_gc_eval
    kGridGtTm = 5,        // k_gt_garble_tm, k_gt_eval_tm: one 160-KiB workgroup per CU
    kGridGtRows = 6,      // k_gt_garble, k_gt_eval (row-major labels)
    kGridFamilies = 7
};
constexpr uint32_t kGridPerCu[kGridFamilies] = {8, 1, 8, 8, 8, 1, 8};
// The one grid rule: `need` workgroups, at most per_cu for each CU of the current device, at least one; a test
// override `cap_blocks` >= 1 (fhh_set_protocol_grid) lowers the device's limit to that many workgroups, 0 leaves it
inline int protocol_grid(uint64_t need, ProtocolGridFamily family, int cap_blocks) {
    uint64_t cap = (uint64_t)device_cus() * kGridPerCu[family];
    if (cap_blocks > 0 && (uint64_t)cap_blocks < cap) cap = (uint64_t)cap_blocks;
    return (int)(need < cap ? (need ? need : 1) : cap);
}
// The launchers below that size their grid by this rule take the ctx's override as `grid_cap` (0: none)
// SoftSpoken GGM trees of both parties from rk / s (one workgroup; before the expands)
hipError_t launch_ss_ggm(const OtArgs& a, hipStream_t stream);
hipError_t launch_ot_recv_expand(const OtArgs& a, hipStream_t stream, int grid_cap);
hipError_t launch_ot_send_expand(const OtArgs& a, hipStream_t stream, int grid_cap);
// the hashes reading T / Q in row form with the transpose fused in (no Tt / Qt pass)
hipError_t launch_ot_send_hash_rows(const OtArgs& a, hipStream_t stream, int grid_cap);
hipError_t launch_ot_recv_hash_rows(const OtArgs& a, hipStream_t stream, int grid_cap);
// *word &= mask (one lane; the tail of a choice-bit buffer)
hipError_t launch_mask_word(uint32_t* word, uint32_t mask, hipStream_t stream);
// the 128 Chou–Orlandi base OTs of OT extension k (fhh_base_ot.cpp)
int base_ot_instance(uint64_t k, const uint8_t seed[32], const uint8_t choices[16], uint8_t* pairs, uint8_t* chosen,
                     std::string* err);
hipError_t launch_ot_level_keys(uint64_t prf, uint32_t level, uint32_t salt, const uint32_t s[4], uint32_t* rk,
                                hipStream_t stream);
// mode 3's second pass (the garbler, FieldElm share): per test t, V = H(q_2t) || H(q_2t+1) (32
// big-endian bytes, sx) mod p255 -> sx pair = V + mask (its node value, a canonical BlockPair), Y0 pair
// ^= (mask ? V + 1 : V - 1); tests = the active OT pairs (ctl-aware as the hashes)
hipError_t launch_cot_fe255_finish(const OtArgs& a, hipStream_t stream, int grid_cap);
// mode 4: the tile-major Q (sender: -> sx) or T (receiver: -> out) as one 16-B row per OT
hipError_t launch_ot_rows_out(const OtArgs& a, bool sender, hipStream_t stream, int grid_cap);
hipError_t launch_gc_garble(const GcArgs& a, hipStream_t stream, int grid_cap);
hipError_t launch_gc_eval(const GcArgs& a, hipStream_t stream, int grid_cap);
hipError_t launch_gt_garble(const GcArgs& a, hipStream_t stream, int grid_cap);   // r05d garbled table
hipError_t launch_gt_eval(const GcArgs& a, hipStream_t stream, int grid_cap);
// sums[c] += the u32 node values vals [C][n] of child c, as u64 (sums zeroed by the caller; Z_2^32 table, b = 3, 4)
hipError_t launch_ring32_child_sums(const uint32_t* vals, uint64_t n, uint64_t C, uint64_t* sums, hipStream_t stream);
hipError_t launch_ring32_child_partials(const uint32_t* vals, uint64_t n, uint64_t G, const LoopCtl* ctl, uint64_t g_off,
                                        uint64_t* partials, uint32_t slot, hipStream_t stream);
hipError_t launch_gather_hist(const uint32_t* sizes, uint32_t stride, const uint32_t* const* rows, uint32_t levels,
                              uint32_t* out, uint64_t cap, hipStream_t stream);
// parity probe of the device loop (fhh_sim_config.probe_*): the pending children's states of a
// client sample, both servers, gathered between k_expand and the count (fhh_loop.hip)
struct ProbeArgs {
    const uint4* seed[2][kMaxDims];     // child tables [E][2][npad] of server s, dim j
    const uint64_t* t[2][kMaxDims];     // [E][2][nw]
    const uint64_t* y[2][kMaxDims];
    const uint32_t* parent_pos;         // [F][d]
    const uint64_t* clients;            // [n_probe] local client indices (< n)
    const LoopCtl* ctl;                 // C (0 once aborted)
    uint4* out_seed;                    // [2][C_cap][n_probe][d][2]
    uint8_t* out_ty;                    // [2][C_cap][n_probe][d][2]: bit0 t, bit1 y
    uint32_t* out_C;                    // C of the level (written unless aborted)
    uint64_t C_cap;
    uint64_t npad, nw;
    uint32_t n_probe, d;
};
hipError_t launch_probe_states(const ProbeArgs& a, hipStream_t stream);
hipError_t launch_loop_init(LoopCtl* ctl, uint32_t d, uint32_t unit, uint32_t max_group, uint32_t max_wpi,
                            uint32_t njobs_per_ctx, uint32_t nctx, uint64_t grid_waves, uint32_t* pos0,
                            uint32_t* live0[kMaxDims], hipStream_t stream);

// ---- sketch + Beaver verification (fhh_sketch.hip), FE values as u64 (any representation) ----
struct SketchArgs {
    const uint8_t* seeds;   // [n_keys][16] PrgStream seeds (sketch_at's rand_stream)
    const uint64_t* x;      // [n_keys][n_nodes]
    const uint64_t* kx;     // [n_keys][n_nodes]
    uint64_t* out;          // [n_keys][6] canonical {r_x, r2_x, r_kx, rand1, rand2, rand3}
    uint64_t n_keys;
    uint32_t n_nodes;
    uint32_t force_sequential;   // 1: every key takes the sequential-stream path (tests)
    uint32_t level;              // the level's stream seed = seed with bytes 12..15 ^= level
    // r05: both servers in one k_sketch_fe launch (the level batch): keys [n_srv, n_keys) are server
    // 1's keys k - n_srv (same seeds, its own x1 / kx1 / out1); n_srv = 0: one server
    uint64_t n_srv;
    const uint64_t* x1;
    const uint64_t* kx1;
    uint64_t* out1;
};
// k_sketch_fe launch plan: keys [0, n_main) at lpk_main lanes per key, the rest at lpk_tail
struct SketchPlan {
    uint64_t n_main;
    int lpk_main, lpk_tail;
};
SketchPlan plan_sketch(uint64_t n_keys, uint32_t n_nodes, uint64_t resident_waves);
// U = FieldElm: values as 8 x u32 little-endian limbs
struct Sketch255Args {
    const uint8_t* seeds;
    const uint32_t* x;      // [n_keys][n_nodes][8]
    const uint32_t* kx;
    uint32_t* out;          // [n_keys][6][8]
    uint64_t n_keys;
    uint32_t n_nodes;
    uint32_t force_sequential;
    uint32_t level;
};
struct Mul255Args {
    const uint32_t* sketch;   // [n][6][8]
    const uint32_t* mac;      // [n][8]
    const uint32_t* mac2;     // [n][8]
    const uint32_t* triples;  // [n][9][8]
    const uint32_t* cor;      // [n][6][8] (mode 1)
    uint32_t* out;            // mode 0: [n][6][8]; mode 1: [n][8]
    uint64_t n;
    uint32_t mode;
    uint32_t server_idx;
};
struct Verify255Args {
    const uint32_t* sketch[2];
    const uint32_t* mac[2];
    const uint32_t* mac2[2];
    const uint32_t* triples[2];
    uint8_t* ok;
    uint32_t* out_shares;     // [2][n][8] or null
    uint64_t n;
};
struct MulArgs {
    const uint64_t* sketch;   // [n][6]
    const uint64_t* mac;      // [n]
    const uint64_t* mac2;     // [n]
    const uint64_t* triples;  // [n][triples_levels][3][a, b, c]
    const uint64_t* cor;      // [n][6] (mode 1)
    uint64_t* out;            // mode 0: [n][6] cor share; mode 1: [n] out share
    uint64_t n;
    uint32_t mode;
    uint32_t server_idx;
    uint32_t level;           // the level's triples (MulState::new's triples[3 level ..], mpc.rs:94-98)
    uint32_t triples_levels;  // levels the triple arrays hold (>= 1)
};
struct VerifyArgs {
    const uint64_t* sketch[2];
    const uint64_t* mac[2];
    const uint64_t* mac2[2];
    const uint64_t* triples[2];
    uint8_t* ok;              // [n]
    uint64_t* out_shares;     // [2][n] or null
    uint64_t n;
    uint32_t level;
    uint32_t triples_levels;
};
hipError_t launch_sketch_fe(const SketchArgs& a, hipStream_t stream);
hipError_t launch_sketch_fe2(const SketchArgs& a, hipStream_t stream, hipStream_t tail_stream);
hipError_t launch_mul_fe(const MulArgs& a, hipStream_t stream);
hipError_t launch_verify_fe(const VerifyArgs& a, hipStream_t stream);
hipError_t launch_deal_triples_fe(uint64_t n, uint32_t levels, uint64_t seed, uint64_t* t0, uint64_t* t1,
                                  hipStream_t stream);
hipError_t launch_sketch_fe255(const Sketch255Args& a, hipStream_t stream);
hipError_t launch_mul_fe255(const Mul255Args& a, hipStream_t stream);
hipError_t launch_verify_fe255(const Verify255Args& a, hipStream_t stream);

}  // namespace fhh
