// Host self-test of csrc/gt_plan.h: the form of a level's GC equality test for every caller (L the device level
// loop, H fhh_gt_cot*_host, P the party ABI), GC form (the loop's cfg->gc 1 / 2 / 3; the party ABI's form 0 / 2 =
// gc 2, form 1 = gc 3), level kind (0 count, 1 FE, 2 FieldElm), bits = 2d (H: 1 .. 4), Z_2^32 request, table_row_major
// and nw = 1, 7, 8, 9, 47, 16 384, against a literal table: the expressions the level loop, gt_cot_host and
// party_begin each spelled out before gt_plan.h existed, evaluated at these inputs (not the function under test).
//   flags  o real_ot, s lshare, t table, m tile_major, w windows, f fused_sums, r ring32,
//          p nw_gc = nw rounded up to 8 words (else nw); npad_gc = 64 nw_gc
//   est    bytes per test of the loop's chunk sizing (0: no such estimate: a count level runs no GC, and H / P
//          size no chunks)
//   "-"    a combination the caller cannot form (form 1 carries no ring request; form 2 is refused at 2d > 4)
// Pinned for the tests that set FHH_GC_CHUNK_BYTES from them: the d = 1 FieldElm estimate 402, the d = 2
// tile-major 320; that the party ABI at bits = 3, 4 is row-major and unfused whatever table_row_major says; and,
// for every row, that no plan is a row-major table at bits <= kGtTmPadBits (those kernels exist at b = 3, 4 only).
#include <cstdio>
#include <cstring>
#include <string>

#include "../../fuzzyheavyhitters_amd/csrc/gt_plan.h"

using fhh::GtCaller;
using fhh::GtPlan;

struct Cell {
    const char* flags;
    uint64_t est;
};
struct Row {
    GtCaller who;
    uint32_t gc, kind, bits, per2;
    Cell cell[4];   // ring 0 rm 0, ring 0 rm 1, ring 1 rm 0, ring 1 rm 1
};
constexpr GtCaller L = GtCaller::kLoop, H = GtCaller::kCotHost, P = GtCaller::kParty;

static const Row kRows[] = {
    {L, 1, 0, 2, 2, {{"", 0}, {"", 0}, {"", 0}, {"", 0}}},
    {L, 1, 0, 4, 2, {{"", 0}, {"", 0}, {"", 0}, {"", 0}}},
    {L, 1, 0, 6, 2, {{"", 0}, {"", 0}, {"", 0}, {"", 0}}},
    {L, 1, 0, 8, 2, {{"", 0}, {"", 0}, {"", 0}, {"", 0}}},
    {L, 1, 1, 2, 1, {{"", 402}, {"", 402}, {"", 402}, {"", 402}}},
    {L, 1, 1, 4, 1, {{"", 802}, {"", 802}, {"", 802}, {"", 802}}},
    {L, 1, 1, 6, 1, {{"", 1202}, {"", 1202}, {"", 1202}, {"", 1202}}},
    {L, 1, 1, 8, 1, {{"", 1602}, {"", 1602}, {"", 1602}, {"", 1602}}},
    {L, 1, 2, 2, 2, {{"", 402}, {"", 402}, {"", 402}, {"", 402}}},
    {L, 1, 2, 4, 2, {{"", 802}, {"", 802}, {"", 802}, {"", 802}}},
    {L, 1, 2, 6, 2, {{"", 1202}, {"", 1202}, {"", 1202}, {"", 1202}}},
    {L, 1, 2, 8, 2, {{"", 1602}, {"", 1602}, {"", 1602}, {"", 1602}}},
    {L, 2, 0, 2, 2, {{"o", 0}, {"o", 0}, {"o", 0}, {"o", 0}}},
    {L, 2, 0, 4, 2, {{"o", 0}, {"o", 0}, {"o", 0}, {"o", 0}}},
    {L, 2, 0, 6, 2, {{"o", 0}, {"o", 0}, {"o", 0}, {"o", 0}}},
    {L, 2, 0, 8, 2, {{"o", 0}, {"o", 0}, {"o", 0}, {"o", 0}}},
    {L, 2, 1, 2, 1, {{"ostmfp", 150}, {"ostmfp", 150}, {"ostmfrp", 150}, {"ostmfrp", 150}}},
    {L, 2, 1, 4, 1, {{"ostmwf", 320}, {"ost", 802}, {"ostmwfr", 320}, {"ostr", 802}}},
    {L, 2, 1, 6, 1, {{"os", 1202}, {"os", 1202}, {"os", 1202}, {"os", 1202}}},
    {L, 2, 1, 8, 1, {{"os", 1602}, {"os", 1602}, {"os", 1602}, {"os", 1602}}},
    {L, 2, 2, 2, 2, {{"o", 402}, {"o", 402}, {"o", 402}, {"o", 402}}},
    {L, 2, 2, 4, 2, {{"o", 802}, {"o", 802}, {"o", 802}, {"o", 802}}},
    {L, 2, 2, 6, 2, {{"o", 1202}, {"o", 1202}, {"o", 1202}, {"o", 1202}}},
    {L, 2, 2, 8, 2, {{"o", 1602}, {"o", 1602}, {"o", 1602}, {"o", 1602}}},
    {L, 3, 0, 2, 2, {{"o", 0}, {"o", 0}, {"o", 0}, {"o", 0}}},
    {L, 3, 0, 4, 2, {{"o", 0}, {"o", 0}, {"o", 0}, {"o", 0}}},
    {L, 3, 0, 6, 2, {{"o", 0}, {"o", 0}, {"o", 0}, {"o", 0}}},
    {L, 3, 0, 8, 2, {{"o", 0}, {"o", 0}, {"o", 0}, {"o", 0}}},
    {L, 3, 1, 2, 1, {{"os", 402}, {"os", 402}, {"os", 402}, {"os", 402}}},
    {L, 3, 1, 4, 1, {{"os", 802}, {"os", 802}, {"os", 802}, {"os", 802}}},
    {L, 3, 1, 6, 1, {{"os", 1202}, {"os", 1202}, {"os", 1202}, {"os", 1202}}},
    {L, 3, 1, 8, 1, {{"os", 1602}, {"os", 1602}, {"os", 1602}, {"os", 1602}}},
    {L, 3, 2, 2, 2, {{"o", 402}, {"o", 402}, {"o", 402}, {"o", 402}}},
    {L, 3, 2, 4, 2, {{"o", 802}, {"o", 802}, {"o", 802}, {"o", 802}}},
    {L, 3, 2, 6, 2, {{"o", 1202}, {"o", 1202}, {"o", 1202}, {"o", 1202}}},
    {L, 3, 2, 8, 2, {{"o", 1602}, {"o", 1602}, {"o", 1602}, {"o", 1602}}},
    {H, 2, 1, 1, 1, {{"ostmp", 0}, {"ostmp", 0}, {"ostmrp", 0}, {"ostmrp", 0}}},
    {H, 2, 1, 2, 1, {{"ostmp", 0}, {"ostmp", 0}, {"ostmrp", 0}, {"ostmrp", 0}}},
    {H, 2, 1, 3, 1, {{"ostmw", 0}, {"ost", 0}, {"ostmwr", 0}, {"ostr", 0}}},
    {H, 2, 1, 4, 1, {{"ostmw", 0}, {"ost", 0}, {"ostmwr", 0}, {"ostr", 0}}},
    {P, 2, 1, 2, 1, {{"ostmfp", 0}, {"ostmfp", 0}, {"ostmfrp", 0}, {"ostmfrp", 0}}},
    {P, 2, 1, 4, 1, {{"ost", 0}, {"ost", 0}, {"ostr", 0}, {"ostr", 0}}},
    {P, 2, 1, 6, 1, {{"os", 0}, {"os", 0}, {"-", 0}, {"-", 0}}},
    {P, 2, 1, 8, 1, {{"os", 0}, {"os", 0}, {"-", 0}, {"-", 0}}},
    {P, 2, 2, 2, 2, {{"o", 0}, {"o", 0}, {"o", 0}, {"o", 0}}},
    {P, 2, 2, 4, 2, {{"o", 0}, {"o", 0}, {"o", 0}, {"o", 0}}},
    {P, 2, 2, 6, 2, {{"o", 0}, {"o", 0}, {"-", 0}, {"-", 0}}},
    {P, 2, 2, 8, 2, {{"o", 0}, {"o", 0}, {"-", 0}, {"-", 0}}},
    {P, 3, 1, 2, 1, {{"os", 0}, {"os", 0}, {"-", 0}, {"-", 0}}},
    {P, 3, 1, 4, 1, {{"os", 0}, {"os", 0}, {"-", 0}, {"-", 0}}},
    {P, 3, 1, 6, 1, {{"os", 0}, {"os", 0}, {"-", 0}, {"-", 0}}},
    {P, 3, 1, 8, 1, {{"os", 0}, {"os", 0}, {"-", 0}, {"-", 0}}},
    {P, 3, 2, 2, 2, {{"o", 0}, {"o", 0}, {"-", 0}, {"-", 0}}},
    {P, 3, 2, 4, 2, {{"o", 0}, {"o", 0}, {"-", 0}, {"-", 0}}},
    {P, 3, 2, 6, 2, {{"o", 0}, {"o", 0}, {"-", 0}, {"-", 0}}},
    {P, 3, 2, 8, 2, {{"o", 0}, {"o", 0}, {"-", 0}, {"-", 0}}},
};

static std::string flags_of(const GtPlan& p, uint64_t nw) {
    std::string f;
    if (p.real_ot) f += 'o';
    if (p.lshare) f += 's';
    if (p.table) f += 't';
    if (p.tile_major) f += 'm';
    if (p.windows) f += 'w';
    if (p.fused_sums) f += 'f';
    if (p.ring32) f += 'r';
    if (p.nw_gc == (nw + 7) / 8 * 8 && p.nw_gc != nw) f += 'p';
    return f;
}

int main() {
    const uint64_t nws[] = {1, 7, 8, 9, 47, 16384};
    int checked = 0;
    for (const Row& r : kRows)
        for (int c = 0; c < 4; c++) {
            const Cell& e = r.cell[c];
            if (!std::strcmp(e.flags, "-")) continue;
            for (uint64_t nw : nws) {
                const GtPlan p = fhh::gt_plan(r.who, r.bits, r.kind, r.gc, c >> 1, c & 1, nw);
                // at a multiple of 8 the padded and the plain pitch coincide: compare without the p
                std::string want = e.flags;
                const bool padded = !want.empty() && want.back() == 'p';
                if (padded && nw % 8 == 0) want.pop_back();
                const uint64_t nw_gc = padded ? (nw + 7) / 8 * 8 : nw;
                if (flags_of(p, nw) != want || p.nw_gc != nw_gc || p.npad_gc != 64 * nw_gc || p.per2 != r.per2 ||
                    (e.est && p.bytes_per_test != e.est)) {
                    std::printf("FAIL caller %d gc %u kind %u bits %u ring %d row_major %d nw %llu: %s nw_gc %llu npad_gc "
                                "%llu per2 %u est %llu, expected %s nw_gc %llu per2 %u est %llu\n",
                                (int)r.who, r.gc, r.kind, r.bits, c >> 1, c & 1, (unsigned long long)nw,
                                flags_of(p, nw).c_str(), (unsigned long long)p.nw_gc, (unsigned long long)p.npad_gc, p.per2,
                                (unsigned long long)p.bytes_per_test, e.flags, (unsigned long long)nw_gc, r.per2,
                                (unsigned long long)e.est);
                    return 1;
                }
                // the row-major table kernels exist at b = 3, 4 only (gt_dispatch refuses the rest)
                if (p.table && !p.tile_major && r.bits <= (uint32_t)fhh::kGtTmPadBits) {
                    std::printf("FAIL caller %d gc %u kind %u bits %u ring %d row_major %d nw %llu: a row-major table at "
                                "b <= %d\n", (int)r.who, r.gc, r.kind, r.bits, c >> 1, c & 1, (unsigned long long)nw,
                                fhh::kGtTmPadBits);
                    return 1;
                }
                checked++;
            }
        }
    // what other tests rely on, by name
    for (int rm = 0; rm < 2; rm++) {
        if (fhh::gt_plan(L, 2, 2, 2, false, rm, 47).bytes_per_test != 402) return std::printf("FAIL 402\n"), 1;
        for (uint32_t bits = 3; bits <= 4; bits++) {
            const GtPlan p = fhh::gt_plan(P, bits, 1, 2, false, rm, 47);
            if (!p.table || p.tile_major || p.fused_sums || p.nw_gc != 47) return std::printf("FAIL party b %u\n", bits), 1;
        }
    }
    if (fhh::gt_plan(L, 4, 1, 2, false, false, 47).bytes_per_test != 320) return std::printf("FAIL 320\n"), 1;
    std::printf("OK %d\n", checked);
    return 0;
}
