// One-shot test entry points of row f1 on host buffers: each packs its byte-per-bit inputs, runs the product
// path of fhh_gcot.cpp (gc_args, ot_run, the GC / table kernels) once on the ctx, and reads the outputs and the
// transcript back in the tests' array-of-structures order.
#include "fhh_engine.h"

#include <algorithm>
#include <cstring>

namespace {

// bits [n][bits] (one byte each, bit 0) -> planes [bits][nw] of 64 tests, then pad_words zero words (the labels
// OT reads the evaluator's planes as its choice words, padded)
std::vector<uint64_t> bit_planes(const uint8_t* src, uint64_t n, uint32_t bits, uint64_t nw, uint64_t pad_words) {
    std::vector<uint64_t> planes((size_t)bits * nw + pad_words, 0);
    for (uint64_t t = 0; t < n; t++)
        for (uint32_t j = 0; j < bits; j++)
            if (src[t * bits + j] & 1) planes[(size_t)j * nw + t / 64] |= 1ull << (t % 64);
    return planes;
}

// m choice bytes (bit 0) -> the OT's padded choice words
std::vector<uint32_t> choice_words(const uint8_t* choices, uint64_t m) {
    std::vector<uint32_t> bits(ot_padded(m) / 32, 0);
    for (uint64_t j = 0; j < m; j++)
        if (choices[j] & 1) bits[j / 32] |= 1u << (j % 32);
    return bits;
}

// SoA [row][stride][16] on the device -> AoS [t][row][16], t < n (dst NULL: not wanted)
int soa_to_aos(fhh_ctx* ctx, const DevBuf& d, uint32_t rows, uint64_t stride, uint64_t n, uint8_t* dst) {
    if (!dst || rows == 0) return FHH_OK;
    std::vector<uint8_t> h((size_t)rows * stride * 16);
    HIP_TRY(ctx, hipMemcpy(h.data(), d.p, h.size(), hipMemcpyDeviceToHost));
    for (uint32_t r = 0; r < rows; r++)
        for (uint64_t t = 0; t < n; t++)
            std::memcpy(dst + (t * rows + r) * 16, h.data() + ((size_t)r * stride + t) * 16, 16);
    return FHH_OK;
}

// the table's messages, SoA [rows][n] of T on the device -> [n][rows] u64 (zero-extended)
template <class T> int msgs_to_aos(fhh_ctx* ctx, const DevBuf& d, uint64_t rows, uint64_t n, uint64_t* msgs) {
    std::vector<T> h(rows * n);
    HIP_TRY(ctx, hipMemcpy(h.data(), d.p, h.size() * sizeof(T), hipMemcpyDeviceToHost));
    for (uint64_t r = 0; r < rows; r++)
        for (uint64_t t = 0; t < n; t++) msgs[t * rows + r] = h[r * n + t];
    return FHH_OK;
}

// one group of n tests on the caller's device buffers (label key and nonce left zero)
fhh_gc_batch gc_batch(uint64_t n, uint64_t nw, uint32_t bits, uint32_t mask, const uint8_t delta[16], uint64_t gate_base,
                      const DevBuf (&dp)[2], const DevBuf& dt, const DevBuf& dg, const DevBuf& de, const DevBuf& dd,
                      const DevBuf& dout) {
    fhh_gc_batch b{};
    b.groups = 1;
    b.clients = (uint32_t)n;
    b.words = (uint32_t)nw;
    b.bits = bits;
    b.mask = mask;
    std::memcpy(b.delta, delta, 16);
    b.gate_base = gate_base;
    b.gb_planes_dev = dp[0].as<uint64_t>();
    b.ev_planes_dev = dp[1].as<uint64_t>();
    b.tables_dev = dt.as<uint8_t>();
    b.gb_labels_dev = dg.as<uint8_t>();
    b.ev_labels_dev = de.as<uint8_t>();
    b.decode_dev = dd.as<uint8_t>();
    b.out_dev = dout.as<uint8_t>();
    return b;
}

}  // namespace

extern "C" {

int fhh_gc_equality_host(fhh_ctx* ctx, uint64_t n, uint32_t bits, const uint8_t* gb_bits, const uint8_t* ev_bits,
                         uint32_t mask, const uint8_t label_key[16], const uint8_t delta[16], uint64_t label_nonce,
                         uint64_t gate_base, uint8_t* tables, uint8_t* gb_labels, uint8_t* ev_labels,
                         uint8_t* decode, uint8_t* out) {
    CTX_CHECK(ctx);
    int rc = ctx_set_device(ctx);
    if (rc) return rc;
    if (bits < 1 || bits > (uint32_t)kGcMaxBits) return ctx->fail(FHH_E_ARG, "gc: bits must be in [1, 8]");
    if (n == 0) return FHH_OK;
    if (!gb_bits || !ev_bits || !label_key || !delta || !out) return ctx->fail(FHH_E_ARG, "gc: NULL argument");
    if (n > 0xFFFFFFFFull) return ctx->fail(FHH_E_ARG, "gc: n must fit 32 bits");
    const uint64_t nw = (n + 63) / 64;
    const std::vector<uint64_t> planes[2] = {bit_planes(gb_bits, n, bits, nw, 0), bit_planes(ev_bits, n, bits, nw, 0)};
    DevBuf dp[2], dt, dg, de, dd, dout;
    for (int s = 0; s < 2; s++) {
        HIP_TRY(ctx, dp[s].ensure(planes[s].size() * 8));
        HIP_TRY(ctx, hipMemcpyAsync(dp[s].p, planes[s].data(), planes[s].size() * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    HIP_TRY(ctx, dt.ensure((size_t)std::max(bits - 1, 1u) * 2 * n * 16));
    HIP_TRY(ctx, dg.ensure((size_t)(bits + 1) * n * 16));
    HIP_TRY(ctx, de.ensure((size_t)bits * n * 16));
    HIP_TRY(ctx, dd.ensure(n));
    HIP_TRY(ctx, dout.ensure(n));
    fhh_gc_batch b = gc_batch(n, nw, bits, mask, delta, gate_base, dp, dt, dg, de, dd, dout);
    std::memcpy(b.label_key, label_key, 16);
    b.label_nonce = label_nonce;
    rc = fhh_gc_equality_device(ctx, &b);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpy(out, dout.p, n, hipMemcpyDeviceToHost));
    if (decode) HIP_TRY(ctx, hipMemcpy(decode, dd.p, n, hipMemcpyDeviceToHost));
    rc = soa_to_aos(ctx, dt, 2 * (bits - 1), n, n, tables);
    if (rc) return rc;
    rc = soa_to_aos(ctx, dg, bits + 1, n, n, gb_labels);
    if (rc) return rc;
    return soa_to_aos(ctx, de, bits, n, n, ev_labels);
}

int fhh_ot_extend_host(fhh_ctx* ctx, uint64_t m, const uint8_t* choices, const uint8_t* x0, const uint8_t* x1,
                       const uint8_t delta[16], const uint8_t base_seeds[128 * 2 * 16], const uint8_t base_choice[16],
                       uint64_t tweak_base, uint8_t* out, uint8_t* u_out, uint8_t* y0_out, uint8_t* y1_out) {
    CTX_CHECK(ctx);
    int rc = ctx_set_device(ctx);
    if (rc) return rc;
    if (m == 0) return FHH_OK;
    if (!choices || !x0 || !out || !base_seeds || !base_choice || (!x1 && !delta))
        return ctx->fail(FHH_E_ARG, "ot_extend: NULL argument");
    const std::vector<uint32_t> bits = choice_words(choices, m);
    uint32_t* ch = nullptr;
    HIP_TRY(ctx, ot_choices_buffer(ctx, m, &ch));
    HIP_TRY(ctx, hipMemcpyAsync(ch, bits.data(), bits.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    DevBuf d0, d1, dout;
    HIP_TRY(ctx, d0.ensure(m * 16));
    HIP_TRY(ctx, dout.ensure(m * 16));
    HIP_TRY(ctx, hipMemcpyAsync(d0.p, x0, m * 16, hipMemcpyHostToDevice, ctx->stream));
    if (x1) {
        HIP_TRY(ctx, d1.ensure(m * 16));
        HIP_TRY(ctx, hipMemcpyAsync(d1.p, x1, m * 16, hipMemcpyHostToDevice, ctx->stream));
    }
    OtOut tr;
    const uint32_t* rk = nullptr;
    rc = ot_host_keys(ctx, base_seeds, base_choice, &rk);
    if (rc) return rc;
    OtArgs a{};
    a.rk = rk;
    words_from_bytes(base_choice, a.s);
    a.choices = ch;
    a.x0 = d0.as<uint4>();
    a.x1 = x1 ? d1.as<uint4>() : nullptr;
    if (!x1) words_from_bytes(delta, a.delta);
    a.out = dout.as<uint4>();
    a.tweak_base = tweak_base;
    rc = ot_run(ctx, a, m, &tr);
    if (rc) return rc;
    rc = ctx_sync(ctx);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpy(out, dout.p, m * 16, hipMemcpyDeviceToHost));
    if (y0_out) HIP_TRY(ctx, hipMemcpy(y0_out, tr.Y0, m * 16, hipMemcpyDeviceToHost));
    if (y1_out) HIP_TRY(ctx, hipMemcpy(y1_out, tr.Y1, m * 16, hipMemcpyDeviceToHost));
    if (u_out) {   // rows [128][ceil(m / 128)] of the padded tile-major matrix
        rc = u_transcript(ctx, tr, m, u_out);
        if (rc) return rc;
    }
    return FHH_OK;
}

int fhh_cot_extend_ss_host(fhh_ctx* ctx, uint32_t ss_k, uint64_t m, uint32_t mode, const uint8_t* choices,
                           const uint8_t delta[16], uint32_t mask, const uint8_t base_seeds[128 * 2 * 16],
                           const uint8_t base_choice[16], uint64_t ctr_off, uint8_t* sender_out, uint8_t* out,
                           uint8_t* u_out, uint8_t* y_out, uint8_t* corr_out) {
    CTX_CHECK(ctx);
    int rc = ctx_set_device(ctx);
    if (rc) return rc;
    if (ss_k != 1 && ss_k != 2 && ss_k != 4) return ctx->fail(FHH_E_ARG, "cot_extend: ss_k must be 1, 2 or 4");
    if (mode < FHH_COT_LABELS || mode > FHH_COT_RAW) return ctx->fail(FHH_E_ARG, "cot_extend: mode must be 1..4");
    if (m == 0) return FHH_OK;
    if (!choices || !out || !base_seeds || !base_choice || (mode == FHH_COT_LABELS && !delta))
        return ctx->fail(FHH_E_ARG, "cot_extend: NULL argument");
    if (mode == FHH_COT_FE255 && (m % 2)) return ctx->fail(FHH_E_ARG, "cot_extend: FieldElm shares take OT pairs (m even)");
    const std::vector<uint32_t> bits = choice_words(choices, m);
    if (mode == FHH_COT_FE255)
        for (uint64_t t = 0; 2 * t < m; t++)
            if (((bits[(2 * t) / 32] >> ((2 * t) % 32)) & 1u) != ((bits[(2 * t + 1) / 32] >> ((2 * t + 1) % 32)) & 1u))
                return ctx->fail(FHH_E_ARG, "cot_extend: a FieldElm OT pair needs one choice for both halves");
    uint32_t* ch = nullptr;
    HIP_TRY(ctx, ot_choices_buffer(ctx, m, &ch));
    HIP_TRY(ctx, hipMemcpyAsync(ch, bits.data(), bits.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    const size_t per = mode == FHH_COT_FE ? 8 : 16;   // bytes per OT of out / sender values / y
    DevBuf dsx, dout;
    HIP_TRY(ctx, dsx.ensure(m * per));
    HIP_TRY(ctx, dout.ensure(m * per));
    const uint32_t* rk = nullptr;
    rc = ot_host_keys(ctx, base_seeds, base_choice, &rk);
    if (rc) return rc;
    OtArgs a{};
    a.mode = mode;
    a.mask = mask & 1u;
    a.rk = rk;
    words_from_bytes(base_choice, a.s);
    a.choices = ch;
    if (delta) words_from_bytes(delta, a.delta);
    a.ctr_off = ctr_off;
    a.sx = dsx.p;
    a.out = dout.as<uint4>();
    a.ss_k = ss_k;
    OtOut tr;
    rc = ot_run(ctx, a, m, &tr);
    if (rc) return rc;
    rc = ctx_sync(ctx);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpy(out, dout.p, m * per, hipMemcpyDeviceToHost));
    if (sender_out) HIP_TRY(ctx, hipMemcpy(sender_out, dsx.p, m * per, hipMemcpyDeviceToHost));
    if (y_out && mode != FHH_COT_RAW) HIP_TRY(ctx, hipMemcpy(y_out, tr.Y0, m * per, hipMemcpyDeviceToHost));
    if (u_out) {
        rc = u_transcript(ctx, tr, m, u_out);
        if (rc) return rc;
    }
    if (corr_out && ss_k > 1) HIP_TRY(ctx, hipMemcpy(corr_out, tr.corr, (size_t)128 * 2 * 16, hipMemcpyDeviceToHost));
    return FHH_OK;
}

int fhh_cot_extend_host(fhh_ctx* ctx, uint64_t m, uint32_t mode, const uint8_t* choices, const uint8_t delta[16],
                        uint32_t mask, const uint8_t base_seeds[128 * 2 * 16], const uint8_t base_choice[16],
                        uint64_t ctr_off, uint8_t* sender_out, uint8_t* out, uint8_t* u_out, uint8_t* y_out) {
    return fhh_cot_extend_ss_host(ctx, 1, m, mode, choices, delta, mask, base_seeds, base_choice, ctr_off, sender_out,
                                  out, u_out, y_out, nullptr);
}

int fhh_gc_cot_host(fhh_ctx* ctx, uint64_t n, uint32_t bits, const uint8_t* gb_bits, const uint8_t* ev_bits,
                    uint32_t mask, uint64_t gate_base, const uint8_t base_seeds[128 * 2 * 16],
                    const uint8_t base_choice[16], uint64_t ctr_off, uint8_t* tables, uint8_t* ev_zero,
                    uint8_t* ev_active, uint8_t* decode, uint8_t* out, uint64_t* gb_share, uint64_t* ev_share,
                    uint64_t* share_y) {
    CTX_CHECK(ctx);
    int rc = ctx_set_device(ctx);
    if (rc) return rc;
    if (bits < 1 || bits > (uint32_t)kGcMaxBits) return ctx->fail(FHH_E_ARG, "gc_cot: bits must be in [1, 8]");
    if (n == 0) return FHH_OK;
    if (!gb_bits || !ev_bits || !base_seeds || !base_choice || !out) return ctx->fail(FHH_E_ARG, "gc_cot: NULL argument");
    if (!(base_choice[0] & 1)) return ctx->fail(FHH_E_ARG, "gc_cot: s is the free-XOR Delta: its bit 0 must be 1");
    if (n > 0xFFFFFFFFull) return ctx->fail(FHH_E_ARG, "gc_cot: n must fit 32 bits");
    const bool share = gb_share || ev_share || share_y;
    if (share && !(gb_share && ev_share && share_y))
        return ctx->fail(FHH_E_ARG, "gc_cot: gb_share, ev_share and share_y go together");
    const uint64_t nw = (n + 63) / 64, npad = 64 * nw, m = (uint64_t)bits * npad;
    const uint64_t pad = ot_padded(m) / 64;   // the evaluator's: OT choice words, padded
    const std::vector<uint64_t> planes[2] = {bit_planes(gb_bits, n, bits, nw, pad), bit_planes(ev_bits, n, bits, nw, pad)};
    DevBuf dp[2], dt, dg, de, da, dd, dout, dsh;
    for (int s = 0; s < 2; s++) {
        HIP_TRY(ctx, dp[s].ensure(planes[s].size() * 8));
        HIP_TRY(ctx, hipMemcpyAsync(dp[s].p, planes[s].data(), planes[s].size() * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    HIP_TRY(ctx, dt.ensure((size_t)std::max(bits - 1, 1u) * 2 * n * 16));
    HIP_TRY(ctx, dg.ensure(16));   // no garbler labels in this protocol (gc_args wants a pointer)
    HIP_TRY(ctx, de.ensure(m * 16));
    HIP_TRY(ctx, da.ensure(m * 16));
    HIP_TRY(ctx, dd.ensure(n));
    HIP_TRY(ctx, dout.ensure(n));
    if (share) HIP_TRY(ctx, dsh.ensure(3 * n * 8));   // [gb | y | ev]
    // 1. the labels OT (OtArgs mode 4): choice bits = the evaluator's planes at OT index j npad + i;
    // the garbler's zero labels q_j, the evaluator's active labels t_j = q_j ^ r_j s
    const uint32_t* rk = nullptr;
    rc = ot_host_keys(ctx, base_seeds, base_choice, &rk);
    if (rc) return rc;
    // Delta = s; no label key: the garbler draws no labels
    const fhh_gc_batch gb = gc_batch(n, nw, bits, mask, base_choice, gate_base, dp, dt, dg, de, dd, dout);
    GcArgs g;
    rc = gc_args(ctx, &gb, g);
    if (rc) return rc;
    OtArgs a{};
    a.mode = 4;
    a.rk = rk;
    words_from_bytes(base_choice, a.s);
    a.choices = dp[1].as<uint32_t>();
    a.ctr_off = ctr_off;
    a.sx = de.p;
    a.out = da.as<uint4>();
    rc = ot_run(ctx, a, m, nullptr);
    if (rc) return rc;
    // 2. garble on the C-OT's zero labels with the garbler's string and mask folded in, 3. evaluate on the
    // OT'd active labels
    g.ev_ot = 1;
    if (share) {
        g.sh_gb = dsh.as<uint64_t>();
        g.sh_y = g.sh_gb + n;
    }
    HIP_TRY(ctx, launch_gc_garble(g, ctx->stream, ctx->protocol_grid));
    g.ev_labels = da.as<uint4>();
    g.sh_gb = nullptr;
    if (share) g.sh_ev = dsh.as<uint64_t>() + 2 * n;
    HIP_TRY(ctx, launch_gc_eval(g, ctx->stream, ctx->protocol_grid));
    rc = ctx_sync(ctx);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpy(out, dout.p, n, hipMemcpyDeviceToHost));
    if (share) {
        HIP_TRY(ctx, hipMemcpy(gb_share, dsh.p, n * 8, hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(share_y, dsh.as<uint64_t>() + n, n * 8, hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(ev_share, dsh.as<uint64_t>() + 2 * n, n * 8, hipMemcpyDeviceToHost));
    }
    if (decode) HIP_TRY(ctx, hipMemcpy(decode, dd.p, n, hipMemcpyDeviceToHost));
    rc = soa_to_aos(ctx, dt, 2 * (bits - 1), n, n, tables);
    if (!rc) rc = soa_to_aos(ctx, de, bits, npad, n, ev_zero);
    if (!rc) rc = soa_to_aos(ctx, da, bits, npad, n, ev_active);
    return rc;
}

static int gt_cot_host(fhh_ctx* ctx, uint64_t n, uint32_t bits, const uint8_t* gb_bits, const uint8_t* ev_bits,
                       uint32_t mask, uint64_t gate_base, const uint8_t base_seeds[128 * 2 * 16],
                       const uint8_t base_choice[16], uint64_t ctr_off, uint8_t* ev_zero, uint8_t* ev_active,
                       uint64_t* msgs, uint64_t* gb_share, uint64_t* ev_share, bool ring32) {
    CTX_CHECK(ctx);
    int rc = ctx_set_device(ctx);
    if (rc) return rc;
    if (bits < 1 || bits > (uint32_t)kGtMaxBits) return ctx->fail(FHH_E_ARG, "gt_cot: bits must be in [1, 4]");
    if (n == 0) return FHH_OK;
    if (!gb_bits || !ev_bits || !base_seeds || !base_choice || !gb_share || !ev_share)
        return ctx->fail(FHH_E_ARG, "gt_cot: NULL argument");
    if (!(base_choice[0] & 1)) return ctx->fail(FHH_E_ARG, "gt_cot: s is the free-XOR Delta: its bit 0 must be 1");
    if (n > 0xFFFFFFFFull) return ctx->fail(FHH_E_ARG, "gt_cot: n must fit 32 bits");
    // the level loop's form of the table (gt_plan.h) at nw = ceil(n / 64); the row-major Z_2^32 kernels'
    // (k_gt_garble<b, true> / k_gt_eval<b, true>) node values are u32
    const GtPlan plan = ctx_gt_plan(ctx, GtCaller::kCotHost, bits, 1, 2, ring32, (n + 63) / 64);
    const bool tm = plan.tile_major;
    const bool val32 = plan.ring32 && !tm;
    const uint64_t nw = plan.nw_gc, npad = plan.npad_gc, m = (uint64_t)bits * npad;
    const uint64_t R = 1ull << bits;
    const uint64_t pad = ot_padded(m) / 64;
    const std::vector<uint64_t> planes[2] = {bit_planes(gb_bits, n, bits, nw, pad), bit_planes(ev_bits, n, bits, nw, pad)};
    DevBuf dp[2], de, da, dm, dsh;
    for (int s = 0; s < 2; s++) {
        HIP_TRY(ctx, dp[s].ensure(planes[s].size() * 8));
        HIP_TRY(ctx, hipMemcpyAsync(dp[s].p, planes[s].data(), planes[s].size() * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    HIP_TRY(ctx, de.ensure(m * 16));
    HIP_TRY(ctx, da.ensure(m * 16));
    HIP_TRY(ctx, dm.ensure(std::max<uint64_t>(R - 1, 1) * n * 8));
    HIP_TRY(ctx, dsh.ensure(2 * n * 8));
    const uint32_t* rk = nullptr;
    rc = ot_host_keys(ctx, base_seeds, base_choice, &rk);
    if (rc) return rc;
    // 1. the labels OT (mode 4, as fhh_gc_cot_host; b <= 2: mode 5, Q / T left tile-major)
    OtArgs a{};
    a.mode = tm ? 5 : 4;
    a.rk = rk;
    words_from_bytes(base_choice, a.s);
    a.choices = dp[1].as<uint32_t>();
    a.ctr_off = ctr_off;
    a.sx = de.p;
    a.out = da.as<uint4>();
    rc = ot_run(ctx, a, m, nullptr);
    if (rc) return rc;
    // 2. the garbled table on the zero labels, 3. its row on the OT'd labels
    GcArgs g{};
    g.gb_planes = dp[0].as<uint64_t>();
    g.ev_planes = dp[1].as<uint64_t>();
    g.G = 1;
    g.N = (uint32_t)n;
    g.nw = (uint32_t)nw;
    g.bits = bits;
    g.mask = mask & 1u;
    words_from_bytes(base_choice, g.delta);
    g.gate_base = gate_base;
    g.ev_labels = tm ? ctx->ot_buf[2].as<uint4>() : de.as<uint4>();
    g.lab_tm = tm ? 1u : 0u;
    g.ev_ot = 1;
    g.gt_msgs = dm.as<uint64_t>();
    g.ring32 = plan.ring32 ? 1u : 0u;
    g.sh_gb = dsh.as<uint64_t>();
    HIP_TRY(ctx, launch_gt_garble(g, ctx->stream, ctx->protocol_grid));
    g.ev_labels = tm ? ctx->ot_buf[0].as<uint4>() : da.as<uint4>();
    g.sh_gb = nullptr;
    g.sh_ev = dsh.as<uint64_t>() + n;
    HIP_TRY(ctx, launch_gt_eval(g, ctx->stream, ctx->protocol_grid));
    if (tm && (ev_zero || ev_active)) {   // the transcript's row-major labels, after the fact (tests only)
        a.m = m;
        a.mp = ot_padded(m);
        a.T = ctx->ot_buf[0].as<uint4>();
        a.Q = ctx->ot_buf[2].as<uint4>();
        HIP_TRY(ctx, launch_ot_rows_out(a, true, ctx->stream, ctx->protocol_grid));
        HIP_TRY(ctx, launch_ot_rows_out(a, false, ctx->stream, ctx->protocol_grid));
    }
    rc = ctx_sync(ctx);
    if (rc) return rc;
    if (val32) {   // u32 values [n] at dsh and at dsh + n u64 (the kernels' sh_gb / sh_ev), zero-extended
        std::vector<uint32_t> h(n);
        uint64_t* dst[2] = {gb_share, ev_share};
        for (int w = 0; w < 2; w++) {
            HIP_TRY(ctx, hipMemcpy(h.data(), dsh.as<uint64_t>() + w * n, n * 4, hipMemcpyDeviceToHost));
            for (uint64_t t = 0; t < n; t++) dst[w][t] = h[t];
        }
    } else {
        HIP_TRY(ctx, hipMemcpy(gb_share, dsh.p, n * 8, hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(ev_share, dsh.as<uint64_t>() + n, n * 8, hipMemcpyDeviceToHost));
    }
    if (msgs && R > 1) {   // the table's rows 1 .. R - 1: u32 in Z_2^32, else u64
        rc = plan.ring32 ? msgs_to_aos<uint32_t>(ctx, dm, R - 1, n, msgs) : msgs_to_aos<uint64_t>(ctx, dm, R - 1, n, msgs);
        if (rc) return rc;
    }
    rc = soa_to_aos(ctx, de, bits, npad, n, ev_zero);
    if (!rc) rc = soa_to_aos(ctx, da, bits, npad, n, ev_active);
    return rc;
}

int fhh_gt_cot_host(fhh_ctx* ctx, uint64_t n, uint32_t bits, const uint8_t* gb_bits, const uint8_t* ev_bits,
                    uint32_t mask, uint64_t gate_base, const uint8_t base_seeds[128 * 2 * 16],
                    const uint8_t base_choice[16], uint64_t ctr_off, uint8_t* ev_zero, uint8_t* ev_active,
                    uint64_t* msgs, uint64_t* gb_share, uint64_t* ev_share) {
    return gt_cot_host(ctx, n, bits, gb_bits, ev_bits, mask, gate_base, base_seeds, base_choice, ctr_off, ev_zero,
                       ev_active, msgs, gb_share, ev_share, false);
}

int fhh_gt_cot_ring32_host(fhh_ctx* ctx, uint64_t n, uint32_t bits, const uint8_t* gb_bits, const uint8_t* ev_bits,
                           uint32_t mask, uint64_t gate_base, const uint8_t base_seeds[128 * 2 * 16],
                           const uint8_t base_choice[16], uint64_t ctr_off, uint8_t* ev_zero, uint8_t* ev_active,
                           uint64_t* msgs, uint64_t* gb_share, uint64_t* ev_share) {
    return gt_cot_host(ctx, n, bits, gb_bits, ev_bits, mask, gate_base, base_seeds, base_choice, ctr_off, ev_zero,
                       ev_active, msgs, gb_share, ev_share, true);
}

}  // extern "C"
