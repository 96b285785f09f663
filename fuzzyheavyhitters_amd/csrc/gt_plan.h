// The form a level's GC equality test takes: which kernels (half-gates circuit or one garbled table per
// test), on which layout of the labels OT's output, with which plane pitch, and who adds the node values
// per child. Decided here for the three host callers (the device level loop in fhh_sim_crawl.cpp, gt_cot_host
// in fhh_gcot_harness.cpp and party_begin in fhh_gcot.cpp). Host-only, no HIP: compiles with any C++17
// compiler; host self-test tests/host/gt_plan_host_test.cpp.
#pragma once
#include <cstdint>

namespace fhh {

constexpr int kGtMaxBits = 4;   // 16 rows (d = 2); wider tests keep the half-gates chain
constexpr int kGtTmMaxBits = 4;   // the table kernels read the tile-major labels (lab_tm) for b <= 4 (d <= 2)
constexpr int kGtTmPadBits = 2;   // b <= 2 (d = 1): plane rows padded to whole 512-client tiles (nw % 8 == 0);
                                  // b = 3, 4 keep Npad = 64 nw, so their OT indices and the wire stay as they were

enum class GtCaller {
    kLoop,      // sim_crawl_device_loop: cfg->gc 1 ideal OT, 2 real OT with the table where it exists, 3 real OT, circuit
    kCotHost,   // fhh_gt_cot_host / fhh_gt_cot_ring32_host: one launch of the table (kind 1, gc 2)
    kParty,     // fhh_gb_* / fhh_ev_*: the ABI's form 0 / 2 = gc 2 (2: Z_2^32 requested), form 1 = gc 3
};

struct GtPlan {
    bool real_ot;      // the evaluator's labels (and the FieldElm level's share) by OT extension
    // r05c: at the FE levels the share comes from the circuit's output labels (no second OT)
    bool lshare;
    // r05d: tests of <= kGtMaxBits bits (d <= 2) take the share from ONE garbled table per test
    // (k_gt_garble / k_gt_eval: 2^bits + 1 AES instead of the half-gates chain's); gc 3: the circuit
    bool table;
    // r06: the table kernels read the labels OT's tile-major Q / T themselves (no k_ot_rows_out)
    bool tile_major;
    // ... on 512-test windows at any nw (b = 3, 4: nw_gc = nw and the OT indices stay); else, tile_major at
    // b <= 2, the plane rows and the OT index take whole 512-client tiles: nw_gc = nw rounded up to 8 words
    bool windows;
    // r06 (tile_major): the kernels add the node values per child into the level's partials themselves (no
    // stored values, no k_child_sums_fe pass)
    bool fused_sums;
    // Z_2^32 table shares in effect (requested, and this level runs the table): the tile-major table, or at
    // b = 3, 4 on the row-major labels k_gt_garble<B, true> / k_gt_eval<B, true> with u32 node values
    bool ring32;
    uint64_t nw_gc, npad_gc;   // plane pitch in 64-client words; the OT index's clients per (child, bit)
    uint32_t per2;             // OTs per test of the share conversion (a FieldElm travels as a BlockPair)
    // chunk sizing (FHH_GC_CHUNK_BYTES / (bytes_per_test x npad) children per chunk): the circuit's GC and OT
    // buffers hold ~400 B per test at d = 1 (200 per bit);
    // r06: the d = 1 garbled table on the tile-major labels holds ~140 B per test (T, U, Q 96, rows 24,
    // node values 16), not the circuit's ~400: larger chunks, one per level at 1M clients;
    // d = 2 on the tile-major labels: T, U, Q 3 x 4 x 16 B and 15 rows of 8 B, ~320 B per test (the row-major
    // path adds both parties' 4 labels and the node values: the circuit's estimate stays).
    // The FieldElm level runs the circuit + share C-OT whatever the FE levels run
    uint64_t bytes_per_test;
};

// bits = 2d; kind = the level's pmode (0 count: no GC, 1 FE, 2 FieldElm = the last level); gc as the loop's
// cfg->gc; ring_req = Z_2^32 shares requested; nw = the ctx's words of 64 clients
inline GtPlan gt_plan(GtCaller who, uint32_t bits, uint32_t kind, uint32_t gc, bool ring_req, bool table_row_major,
                      uint64_t nw) {
    GtPlan p{};
    p.real_ot = gc >= 2;
    p.lshare = p.real_ot && kind == 1;
    p.table = p.lshare && bits <= (uint32_t)kGtMaxBits && gc == 2;
    // fhh_set_table_row_major keeps b = 3, 4 on k_ot_rows_out's row-major labels (the A/B partner)
    p.tile_major = p.table && bits <= (uint32_t)kGtTmMaxBits && (bits <= (uint32_t)kGtTmPadBits || !table_row_major);
    // the party ABI keeps the row-major labels at b = 3, 4, whatever fhh_set_table_row_major says: a tile-major
    // party run once produced a wrong gc message and the cause was not found (the tile-major kernels of that
    // width serve the level loop and fhh_gt_cot*_host only)
    if (who == GtCaller::kParty && bits > (uint32_t)kGtTmPadBits) p.tile_major = false;
    p.windows = p.tile_major && bits > (uint32_t)kGtTmPadBits;
    // r06: the tile-major table kernels add the node values per child themselves (fhh_gt_cot*_host returns every
    // test's shares)
    p.fused_sums = p.tile_major && who != GtCaller::kCotHost;
    p.ring32 = ring_req && p.table && bits <= (uint32_t)kGtTmMaxBits;
    p.nw_gc = p.tile_major && !p.windows ? (nw + 7) / 8 * 8 : nw;
    p.npad_gc = 64 * p.nw_gc;
    p.per2 = kind == 1 ? 1 : 2;
    p.bytes_per_test = !p.tile_major ? 200ull * bits + 2 : p.windows ? 320 : 150;
    return p;
}

}  // namespace fhh
