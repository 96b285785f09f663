// The in-process two-server harness: both servers' ctxs on one GPU and one stream (PairScope). fhh_sim_eq_count
// and fhh_sim_ot_sums test one pending level; fhh_sim_crawl runs a whole crawl, level by level from the host
// (host_loop) or as the device-resident level loop with its GC + OT chunks and base-OT producer threads.
#include "fhh_engine.h"

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <mutex>
#include <optional>
#include <thread>

namespace {

int check_pair(fhh_ctx* c0, fhh_ctx* c1) {
    if (!c0 || !c1) {
        g_err = "null fhh_ctx";
        return FHH_E_ARG;
    }
    if (c0->device != c1->device) return c0->fail(FHH_E_ARG, "sim: ctxs on different devices");
    if (c0->d != c1->d || c0->n != c1->n || c0->L != c1->L)
        return c0->fail(FHH_E_ARG, "sim: ctx shapes differ");
    if (c0->phase != c1->phase || (c0->phase != Phase::kPending && c0->phase != Phase::kPendingLast))
        return c0->fail(FHH_E_STATE, "sim: both ctxs need a pending crawl");
    if (c0->pending_C != c1->pending_C || c0->frontier.size() != c1->frontier.size())
        return c0->fail(FHH_E_ARG, "sim: frontiers differ");
    for (size_t k = 0; k < c0->frontier.size(); k++)
        for (uint32_t j = 0; j < c0->d; j++)
            if (c0->frontier[k].pos[j] != c1->frontier[k].pos[j]) return c0->fail(FHH_E_ARG, "sim: frontiers differ");
    if (c1->stream != c0->stream) HIP_TRY(c1, hipStreamSynchronize(c1->stream));
    return FHH_OK;
}

// partials on device -> (optional all-reduce) -> host
int fetch_partials(fhh_ctx* ctx, const fhh_sim_config* cfg, uint64_t* dev, uint64_t count, uint64_t* host) {
    if (count == 0) return FHH_OK;
    if (cfg && cfg->comm) {
        std::string err;
        if (comm_allreduce(cfg->comm, dev, dev, count, ctx->stream, &err)) return ctx->fail(FHH_E_COMM, err);
        HIP_TRY(ctx, hipMemcpyAsync(host, dev, count * 8, hipMemcpyDeviceToHost, ctx->stream));
    } else if (cfg && cfg->allreduce) {
        if (!cfg->xchg_dev || cfg->xchg_capacity < count)
            return ctx->fail(FHH_E_ARG, "sim: all-reduce exchange buffer too small");
        HIP_TRY(ctx, hipMemcpyAsync(cfg->xchg_dev, dev, count * 8, hipMemcpyDeviceToDevice, ctx->stream));
        int rc = ctx_sync(ctx);
        if (rc) return rc;
        if (cfg->allreduce(cfg->xchg_dev, count, cfg->allreduce_user) != 0)
            return ctx->fail(FHH_E_CALLBACK, "all-reduce callback failed");
        HIP_TRY(ctx, hipMemcpyAsync(host, cfg->xchg_dev, count * 8, hipMemcpyDeviceToHost, ctx->stream));
    } else {
        HIP_TRY(ctx, hipMemcpyAsync(host, dev, count * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    return ctx_sync(ctx);
}

int sim_eq_count_impl(fhh_ctx* c0, fhh_ctx* c1, const fhh_sim_config* cfg, uint64_t* counts) {
    int rc = check_pair(c0, c1);
    if (rc) return rc;
    const uint64_t C = c0->pending_C;
    HIP_TRY(c0, c0->scratch2.ensure(std::max<uint64_t>(C, 1) * 8 * 16));
    ChildArgs a = child_args(c0, c1);
    HIP_TRY(c0, launch_eq_count(a, c0->scratch2.as<uint64_t>(), c0->stream));
    return fetch_partials(c0, cfg, c0->scratch2.as<uint64_t>(), C, counts);
}

// mode FE (non-last): sums0/sums1 [C] canonical; FE255 (last): [C][10] unreduced
int sim_ot_sums_impl(fhh_ctx* c0, fhh_ctx* c1, const fhh_sim_config* cfg, uint64_t seed, void* s0, void* s1) {
    int rc = check_pair(c0, c1);
    if (rc) return rc;
    const uint64_t C = c0->pending_C;
    const bool last = c0->phase == Phase::kPendingLast;
    const uint64_t per = last ? 16 : 4;
    HIP_TRY(c0, c0->scratch2.ensure(std::max<uint64_t>(C, 1) * 8 * 16));
    ChildArgs a = child_args(c0, c1);
    a.prf_seed = seed;
    if (last) HIP_TRY(c0, launch_child_sums_fe255(a, c0->scratch2.as<uint64_t>(), c0->stream));
    else HIP_TRY(c0, launch_child_sums_fe(a, c0->scratch2.as<uint64_t>(), c0->stream, true));
    std::vector<uint64_t> h(C * per);
    rc = fetch_partials(c0, cfg, c0->scratch2.as<uint64_t>(), C * per, h.data());
    if (rc) return rc;
    for (uint64_t c = 0; c < C; c++) {
        if (!last) {
            static_cast<uint64_t*>(s0)[c] = fe_canon_from_limbs(h[c * 4 + 0], h[c * 4 + 1]);
            static_cast<uint64_t*>(s1)[c] = fe_canon_from_limbs(h[c * 4 + 2], h[c * 4 + 3]);
        } else {
            Limbs10 v0 = limbs_from_partials(&h[c * 16]);
            Limbs10 v1 = limbs_from_partials(&h[c * 16 + 8]);
            std::memcpy(static_cast<uint32_t*>(s0) + c * 10, v0.data(), 40);
            std::memcpy(static_cast<uint32_t*>(s1) + c * 10, v1.data(), 40);
            c0->last_values[c] = v0;
            c1->last_values[c] = v1;
        }
    }
    return FHH_OK;
}

}  // namespace

// ---- device-resident level loop (fhh_sim_crawl, host_loop = 0) ---------------------------------
// FHH_DEBUG_PHASES=1 prints host wall-clock per crawl phase to stderr (setup / loop / readback)
struct PhaseClock {
    bool on = std::getenv("FHH_DEBUG_PHASES") != nullptr;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void mark(const char* what) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[fhh phase] %-10s %9.3f ms\n", what,
                     std::chrono::duration<double, std::milli>(now - t).count());
        t = now;
    }
};

// Host producer of the real base OTs (fhh_sim_config.base_ot). Each level's two OT extensions — kind
// 0 the evaluator's labels, kind 1 the share conversion — start from their own 128 Chou–Orlandi OTs
// (AlszSender/AlszReceiver::init per channel and level, collect.rs:454-471); the level's chunks extend
// them from disjoint row-PRG counters. The level loop requests instances (lv, kind) a few levels ahead
// of the level it enqueues; worker threads compute them in request order with their key schedules
// [3][128][44] (receiver k_i^0, k_i^1; sender k_i^{s_i}); wait(i) blocks until request i is done.
// Accounting (fhh_stats): compute_ms sums every instance's own CO15 + key-schedule time over the
// workers (the host CPU the base OTs cost), stall_ms is the time the enqueueing thread spent blocked
// in wait() — the base OTs' share of the crawl's critical path. An instance's schedules are released
// once uploaded (release()); a resumed level re-requests and recomputes them.
struct BaseOtProducer {
    struct Inst {
        uint32_t lv, salt;
        std::vector<uint32_t> rk;
        bool done = false;
    };
    uint64_t prf;
    uint8_t seed[32];
    std::deque<Inst> insts;                          // stable addresses under push_back
    std::map<uint64_t, size_t> index;                // (lv << 32 | salt) -> request (until released)
    size_t next_work = 0;
    bool stop = false;
    std::mutex mu;
    std::condition_variable cv_done, cv_work;
    int rc = FHH_OK;
    std::string err;
    std::vector<std::thread> workers;
    double compute_ms = 0;                           // summed per-instance compute (all workers)
    double stall_ms = 0;                             // enqueueing thread blocked in wait()
    uint64_t computed = 0;                           // instances finished
    BaseOtProducer(uint64_t prf_seed, const uint8_t s[32]) : prf(prf_seed) {
        std::memcpy(seed, s, 32);
        unsigned nt = std::thread::hardware_concurrency();
        if (const char* e = std::getenv("OMP_NUM_THREADS")) nt = (unsigned)std::atoi(e);
        nt = std::max(1u, std::min(nt ? nt : 1u, 64u));
        for (unsigned w = 0; w < nt; w++) workers.emplace_back([this] { work(); });
    }
    ~BaseOtProducer() {
        {
            std::lock_guard<std::mutex> lk(mu);
            stop = true;
        }
        cv_work.notify_all();
        for (auto& t : workers) t.join();
    }
    size_t request(uint32_t lv, uint32_t salt) {
        std::lock_guard<std::mutex> lk(mu);
        const uint64_t key = (uint64_t)lv << 32 | salt;
        auto it = index.find(key);
        if (it != index.end()) return it->second;
        insts.push_back(Inst{lv, salt, {}, false});
        index.emplace(key, insts.size() - 1);
        cv_work.notify_one();
        return insts.size() - 1;
    }
    void work() {
        std::vector<uint8_t> pairs(128 * 32), chosen(128 * 16);
        for (;;) {
            Inst* in = nullptr;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv_work.wait(lk, [&] { return stop || next_work < insts.size(); });
                if (stop) return;
                in = &insts[next_work++];
            }
            const auto t_begin = std::chrono::steady_clock::now();
            // the OT-extension sender's base choice bits: the words the ideal mode uses (ot_level_choice)
            uint32_t sw[4];
            ot_level_choice(prf, in->lv, in->salt, sw);
            uint8_t ch[16];
            std::memcpy(ch, sw, 16);
            std::string e;
            const int r = base_ot_instance((uint64_t)in->lv << 32 | in->salt, seed, ch, pairs.data(), chosen.data(), &e);
            std::vector<uint32_t> rk;
            if (!r) {
                rk.resize((size_t)3 * 128 * 44);
                base_ot_schedules(pairs.data(), chosen.data(), rk.data());
            }
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
            std::lock_guard<std::mutex> lk(mu);
            if (r && !rc) {
                rc = r;
                err = e;
            }
            in->rk.swap(rk);
            in->done = true;
            compute_ms += ms;
            computed++;
            cv_done.notify_all();
        }
    }
    int wait(size_t i) {
        std::unique_lock<std::mutex> lk(mu);
        if (insts[i].done || rc != FHH_OK) return rc;
        const auto t_begin = std::chrono::steady_clock::now();
        cv_done.wait(lk, [&] { return insts[i].done || rc != FHH_OK; });
        stall_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
        return rc;
    }
    const uint32_t* schedules(size_t i) {
        std::lock_guard<std::mutex> lk(mu);
        return insts[i].rk.data();
    }
    // the schedules have left the host (their upload returned): free them, and let a later request for
    // the same (lv, salt) compute a fresh instance
    void release(size_t i) {
        std::lock_guard<std::mutex> lk(mu);
        std::vector<uint32_t>().swap(insts[i].rk);
        index.erase((uint64_t)insts[i].lv << 32 | insts[i].salt);
    }
};

struct LoopBuffers {
    DevBuf ctl, live[2], pos[2], mark, partials, sizes, final_vals;
    DevBuf hist_rows, hist_packed;               // end-of-crawl readback (k_gather_hist)
    DevBuf gc_planes[2], gc_tables, gc_gbl, gc_evl, gc_decode, gc_out;   // cfg->gc (row f1)
    DevBuf gc_evact, gc_val[2], gc_y, gc_msgs;                            // cfg->gc = 2: OT / share / table buffers
    // multi-rank: kernels write this rank's partials, k_prune reads the cross-rank sum in
    // `reduced` (out of place, so re-reducing an aborted level's stale partials is idempotent)
    DevBuf reduced;
    DevBuf agree;                                // multi-rank: the growth decision's flags (loop_entry_cap)
    bool distributed = false;
    uint64_t* red() const { return distributed ? reduced.as<uint64_t>() : partials.as<uint64_t>(); }
    // parity probe (cfg->probe_*): per probed level, the gathered states at stride probe_stride
    static constexpr uint32_t kMaxProbe = 16;
    DevBuf probe_seed[kMaxProbe], probe_ty[kMaxProbe];
    uint64_t probe_stride[kMaxProbe] = {};
    DevBuf probe_C, probe_clients;
    // cfg->base_ot: the key schedules [3][128][44] of the real base OTs, uploaded into a ring of
    // kBaseRing slots on the engine stream (stream order: a slot is rewritten only after the OT
    // kernels enqueued before the copy have read it)
    static constexpr uint32_t kBaseRing = 8;
    bool base_ot = false;
    DevBuf base_rk;
    uint32_t base_slot = 0;
    std::unique_ptr<BaseOtProducer> bot;
    std::vector<DevBuf*> hist_epochs;            // hist rows; a new epoch per F_cap growth
    std::vector<uint32_t*> hist_ptr;             // per level
    uint32_t E_cap = 0, F_cap = 0;
    PinnedBuf ctl_host, rec;                     // ctl readback; per-level partial records
    std::vector<size_t> rec_off;                 // per level offset (u64) into rec
    std::vector<uint32_t> rec_stride;            // per level C_cap at that time
    ~LoopBuffers() {
        for (auto* b : hist_epochs) delete b;
    }
};

// one device-loop crawl: what its phases (loop_setup .. loop_probe_readback) share
struct Loop : LoopBuffers {
    fhh_ctx *c0, *c1, *cs[2];
    const fhh_sim_config* cfg;
    uint32_t levels, d;
    int variant;
    uint64_t grid_waves;
    uint64_t thr;
    uint32_t thr_last;
    // GC + OT chunk: children per protocol instance, so the level's GC and OT buffers (GtPlan::bytes_per_test
    // per test) stay within FHH_GC_CHUNK_BYTES (default 64 GiB): one chunk per level at configs[1], ~160
    // children per chunk at 1M clients
    uint64_t gc_budget = 64ull << 30;
    bool record;   // cfg->counts: every level's reduced partials are kept for the host
    std::optional<PairScope> pair;   // from loop_setup's tree_init on, both servers run on c0's stream
    Loop(fhh_ctx* a, fhh_ctx* b, const fhh_sim_config* cf, uint32_t lvls, uint64_t t, uint32_t tl)
        : c0(a), c1(b), cs{a, b}, cfg(cf), levels(lvls), d(a->d), variant(a->variant),
          grid_waves((uint64_t)a->grid * (expand_threads(a->variant) / 64)), thr(t), thr_last(tl),
          record(cf->counts != nullptr) {
        distributed = cf->comm || cf->allreduce;
        if (const char* e = std::getenv("FHH_GC_CHUNK_BYTES")) gc_budget = std::strtoull(e, nullptr, 10);
    }
    // the form of level kind `pmode`'s equality tests (gt_plan.h)
    GtPlan plan(uint32_t pmode) const {
        return ctx_gt_plan(c0, GtCaller::kLoop, 2 * d, pmode, cfg->gc, cfg->table_ring32 != 0, c0->nw);
    }
};

// one level of the crawl as its phases see it
struct Level {
    uint32_t lv;
    bool last;
    int par;          // table buffer of the level's parents; the children go to 1 - par
    uint32_t pmode;   // 0 counts, 1 FE, 2 FieldElm (the last level)
    uint32_t per;     // partial u64 per child
    uint64_t C_cap;   // children the buffers hold: grid hint and all-reduce count (the real C is in LoopCtl)
    bool timed;       // this level's launches are event-timed (fhh_set_timing)
    Level(const Loop& S, uint32_t l)
        : lv(l), last(l + 1 == S.levels), par(l & 1), pmode(S.cfg->mode == 0 ? 0 : (last ? 2 : 1)),
          per(pmode == 0 ? 1 : (pmode == 1 ? 4 : 16)), C_cap((uint64_t)S.F_cap << S.d),
          timed(S.c0->timing && l % S.c0->timing_every == 0) {}
};

// wait for the base OTs of OT extension (lv, salt) and copy their key schedules to the next ring
// slot; returns the slot's device address. The copy is from pageable memory, so it has left the host
// buffer on return, and the instance is released.
int upload_base_ot(fhh_ctx* c0, LoopBuffers& B, uint32_t lv, uint32_t salt, const uint32_t** rk_dev) {
    const size_t i = B.bot->request(lv, salt);
    const int rc = B.bot->wait(i);
    if (rc) return c0->fail(rc, "base OTs: " + B.bot->err);
    const size_t words = (size_t)3 * 128 * 44;
    uint32_t* dst = B.base_rk.as<uint32_t>() + (size_t)(B.base_slot++ % LoopBuffers::kBaseRing) * words;
    HIP_TRY(c0, hipMemcpyAsync(dst, B.bot->schedules(i), words * 4, hipMemcpyHostToDevice, c0->stream));
    B.bot->release(i);   // a pageable copy has left the host buffer on return
    *rk_dev = dst;
    return FHH_OK;
}

uint32_t next_pow2(uint32_t v) {
    uint32_t p = 1;
    while (p < v) p <<= 1;
    return p;
}

// grow one buffer of a dim table, preserving the first `keep` entries
int table_grow(fhh_ctx* ctx, DimTable& T, int buf, size_t cap, size_t keep) {
    if (cap <= T.cap[buf] && T.seed[buf].p) return FHH_OK;
    DevBuf ns, nt, ny;
    HIP_TRY(ctx, ns.ensure(cap * 2 * ctx->npad * 16));
    HIP_TRY(ctx, nt.ensure(cap * 2 * ctx->nw * 8));
    HIP_TRY(ctx, ny.ensure(cap * 2 * ctx->nw * 8));
    if (keep) {
        HIP_TRY(ctx, hipMemcpyAsync(ns.p, T.seed[buf].p, keep * 2 * ctx->npad * 16, hipMemcpyDeviceToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(nt.p, T.t[buf].p, keep * 2 * ctx->nw * 8, hipMemcpyDeviceToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(ny.p, T.y[buf].p, keep * 2 * ctx->nw * 8, hipMemcpyDeviceToDevice, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    T.seed[buf].swap(ns);
    T.t[buf].swap(nt);
    T.y[buf].swap(ny);
    T.cap[buf] = cap;
    return FHH_OK;
}

void table_release(DimTable& T, int buf) {
    T.seed[buf].release();
    T.t[buf].release();
    T.y[buf].release();
    T.cap[buf] = 0;
}

size_t table_entry_bytes(const fhh_ctx* c) { return 2 * c->npad * 16 + 2 * 2 * c->nw * 8; }

// Entry capacity of every dim table after a device-loop abort that needs `need` entries. 2x the
// next power of two (few resumes) when the tables of the servers on this device fit beside what
// else is allocated; else 1.25x the need in 64-entry steps; else the need itself. At 1M clients an
// entry is 32 MB (both sides' seeds), so the doubling alone overshot 288 GB at configs[3]'s dense
// thresholds (2 servers x d dims x 2 parities of tables on one GPU).
//
// Ranks of a sharded crawl (cfg->comm / cfg->allreduce) must pick the SAME capacity: the abort level
// of every later batch, the loop's all-reduce sequence and count (C_cap x per) and the next crawl's
// loop_cap_hint all follow from it, and their free memory differs. So each rank's "does candidate k
// fit here" flags are summed over the ranks through the loop's own reduction and the first candidate
// that fits on every rank is taken. FHH_TEST_TABLE_BYTES="a0,a1,..." replaces the available bytes of
// rank r by a_r (the last entry for higher ranks): r = the communicator's rank, or FHH_TEST_RANK on the
// cfg->allreduce callback path (0 if unset): tests force different free memory per rank with it.
// all-reduce `count` u64 from src into dst on the engine stream, over the crawl's transport: the
// communicator (cfg->comm), or the cfg->allreduce callback on the exchange buffer, which runs on the host:
// the stream is drained before it
int loop_allreduce(Loop& S, const uint64_t* src, uint64_t* dst, uint64_t count) {
    fhh_ctx* c0 = S.c0;
    const fhh_sim_config* cfg = S.cfg;
    if (cfg->comm) {
        std::string err;
        if (comm_allreduce(cfg->comm, src, dst, count, c0->stream, &err)) return c0->fail(FHH_E_COMM, err);
        return FHH_OK;
    }
    if (!cfg->xchg_dev || cfg->xchg_capacity < count)
        return c0->fail(FHH_E_ARG, "sim: all-reduce exchange buffer too small");
    HIP_TRY(c0, hipMemcpyAsync(cfg->xchg_dev, src, count * 8, hipMemcpyDeviceToDevice, c0->stream));
    const int rc = ctx_sync(c0);
    if (rc) return rc;
    if (cfg->allreduce(cfg->xchg_dev, count, cfg->allreduce_user) != 0)
        return c0->fail(FHH_E_CALLBACK, "all-reduce callback failed");
    HIP_TRY(c0, hipMemcpyAsync(dst, cfg->xchg_dev, count * 8, hipMemcpyDeviceToDevice, c0->stream));
    return FHH_OK;
}

int loop_entry_cap(Loop& B, uint32_t need, uint32_t la, uint32_t& out) {
    fhh_ctx* const(&cs)[2] = B.cs;
    const fhh_sim_config* cfg = B.cfg;
    const uint32_t d = B.d, E_cap = B.E_cap;
    size_t free_b = 0, total_b = 0;
    HIP_TRY(cs[0], hipMemGetInfo(&free_b, &total_b));
    size_t held = 0, old_pres = 0, n_tab = 0;   // bytes the tables hold now; largest preserved one
    for (fhh_ctx* c : cs) {
        if (c->device != cs[0]->device) continue;
        const size_t bpe = table_entry_bytes(c);
        for (uint32_t j = 0; j < d; j++) {
            held += (c->tab[j].cap[0] + c->tab[j].cap[1]) * bpe;
            old_pres = std::max(old_pres, c->tab[j].cap[1 - (la & 1)] * bpe);
            n_tab += 2;
        }
    }
    const size_t bpe = table_entry_bytes(cs[0]);
    const size_t margin = (size_t)2 << 30;
    size_t avail = free_b + held > margin ? free_b + held - margin : 0;
    if (const char* e = std::getenv("FHH_TEST_TABLE_BYTES")) {
        const char* tr = std::getenv("FHH_TEST_RANK");
        const int r = cfg->comm ? comm_rank(cfg->comm) : (tr ? std::atoi(tr) : 0);
        std::string s(e);
        size_t pos = 0;
        for (int k = 0;; k++) {
            const size_t comma = s.find(',', pos);
            avail = (size_t)std::strtoull(s.substr(pos, comma - pos).c_str(), nullptr, 10);
            if (k == r || comma == std::string::npos) break;
            pos = comma + 1;
        }
    }
    const uint64_t cand[3] = {(uint64_t)next_pow2(need) * 2, ((uint64_t)need * 5 / 4 + 63) / 64 * 64, need};
    uint64_t nofit[3];
    for (int k = 0; k < 3; k++) {
        const uint64_t e = std::max<uint64_t>(cand[k], E_cap);
        nofit[k] = e * bpe * n_tab + old_pres <= avail ? 0 : 1;
    }
    if (cfg->comm || cfg->allreduce) {
        // every rank reaches this abort at the same level (the frontier is replicated and the
        // capacities agree), so the extra collective pairs up across ranks
        fhh_ctx* c0 = cs[0];
        HIP_TRY(c0, B.agree.ensure(2 * 3 * 8));
        uint64_t* dv = B.agree.as<uint64_t>();
        HIP_TRY(c0, hipMemcpyAsync(dv, nofit, sizeof nofit, hipMemcpyHostToDevice, c0->stream));
        const int rc = loop_allreduce(B, dv, dv + 3, 3);
        if (rc) return rc;
        HIP_TRY(c0, hipMemcpyAsync(nofit, dv + 3, sizeof nofit, hipMemcpyDeviceToHost, c0->stream));
        HIP_TRY(c0, hipStreamSynchronize(c0->stream));
    }
    out = std::max<uint32_t>(E_cap, need);
    for (int k = 0; k < 3; k++)
        if (!nofit[k]) {
            out = (uint32_t)std::max<uint64_t>(cand[k], E_cap);
            break;
        }
    if (std::getenv("FHH_DEBUG_LOOP"))
        std::fprintf(stderr, "[fhh loop] entry cap: need %u -> %u (%.1f GB of tables, %.1f GB available)\n", need,
                     out, (double)out * bpe * n_tab / 1e9, (double)avail / 1e9);
    return FHH_OK;
}

// (re)size the loop buffers; preserve what a resumed prune of `level` still reads, and with keep_live (the dims'
// n_live) the live lists `level` was expanded from: the last level's, which loop_readback hands to the engine
int loop_resize(fhh_ctx* c0, LoopBuffers& B, uint32_t E_cap, uint32_t F_cap, uint32_t levels, uint32_t level,
                bool preserve, uint32_t keep_nodes, uint32_t keep_children, uint32_t per,
                const uint32_t* keep_live = nullptr) {
    const uint32_t d = c0->d;
    const size_t C_new = (size_t)F_cap << d;
    HIP_TRY(c0, hipStreamSynchronize(c0->stream));
    for (int b = 0; b < 2; b++) {
        const int keep_par = level & 1;
        DevBuf nl;
        HIP_TRY(c0, nl.ensure((size_t)d * E_cap * 4));
        if (preserve && b == keep_par && keep_live) {
            for (uint32_t j = 0; j < d; j++)
                if (keep_live[j])
                    HIP_TRY(c0, hipMemcpyAsync(nl.as<uint32_t>() + (size_t)j * E_cap,
                                               B.live[b].as<uint32_t>() + (size_t)j * B.E_cap, (size_t)keep_live[j] * 4,
                                               hipMemcpyDeviceToDevice, c0->stream));
            HIP_TRY(c0, hipStreamSynchronize(c0->stream));
        }
        B.live[b].swap(nl);
        DevBuf np;
        HIP_TRY(c0, np.ensure((size_t)F_cap * d * 4));
        if (preserve && b == keep_par && keep_nodes) {
            // stream-ordered (the engine streams do not wait for the null stream), and finished
            // before the old buffer is released
            HIP_TRY(c0, hipMemcpyAsync(np.p, B.pos[b].p, (size_t)keep_nodes * d * 4, hipMemcpyDeviceToDevice, c0->stream));
            HIP_TRY(c0, hipStreamSynchronize(c0->stream));
        }
        B.pos[b].swap(np);
    }
    HIP_TRY(c0, B.mark.ensure((size_t)d * E_cap * 4));
    {
        // a resumed prune reads the (reduced) partials of `level`
        DevBuf npart, nred;
        HIP_TRY(c0, npart.ensure(C_new * 16 * 8));
        // FE levels add into the partials (k_child_sums_fe client chunks); k_prune re-zeroes them
        HIP_TRY(c0, hipMemsetAsync(npart.p, 0, C_new * 16 * 8, c0->stream));
        if (B.distributed) HIP_TRY(c0, nred.ensure(C_new * 16 * 8));
        // ... and, multi-rank, the local partials too: the all-reduces of the no-op levels
        // after an abort re-reduce them, which must reproduce the same sums
        if (preserve && keep_children) {
            HIP_TRY(c0, hipMemcpyAsync(npart.p, B.partials.p, (size_t)keep_children * per * 8, hipMemcpyDeviceToDevice, c0->stream));
            if (B.distributed)
                HIP_TRY(c0, hipMemcpyAsync(nred.p, B.reduced.p, (size_t)keep_children * per * 8, hipMemcpyDeviceToDevice, c0->stream));
        }
        HIP_TRY(c0, hipStreamSynchronize(c0->stream));
        B.partials.swap(npart);
        if (B.distributed) B.reduced.swap(nred);
    }
    // hist rows for levels >= level live in a new epoch of stride F_cap
    DevBuf* ep = new DevBuf();
    if (ep->ensure((size_t)(levels - level) * F_cap * 4) != hipSuccess) {
        delete ep;
        return c0->fail(FHH_E_NOMEM, "loop: hist allocation failed");
    }
    B.hist_epochs.push_back(ep);
    B.hist_ptr.resize(levels, nullptr);
    for (uint32_t lv = level; lv < levels; lv++) B.hist_ptr[lv] = ep->as<uint32_t>() + (size_t)(lv - level) * F_cap;
    B.E_cap = E_cap;
    B.F_cap = F_cap;
    return FHH_OK;
}

// ---- the device level loop's phases, in the order sim_crawl_device_loop runs them ----

// table growth, tree_init of both servers, the ctl / sizes / probe buffers, the base-OT producer, k_loop_init
int loop_setup(Loop& S) {
    fhh_ctx *c0 = S.c0, *c1 = S.c1;
    const fhh_sim_config* cfg = S.cfg;
    const uint32_t d = S.d, levels = S.levels;
    uint32_t cap0 = std::max(cfg->init_capacity ? next_pow2(cfg->init_capacity) : 256u, c0->loop_cap_hint);
    // keys still staged by fhh_add_keys go to the device first: until then npad is 0, and the tables grown
    // below would be sized for no client while tree_init's roots are npad wide
    for (fhh_ctx* c : S.cs)
        if (c->h_n) {
            const int rc = fhh_tree_init(c);
            if (rc) return rc;
        }
    // tables: both buffers of every dim of both servers hold >= E_cap entries
    for (fhh_ctx* c : S.cs)
        for (uint32_t j = 0; j < d; j++)
            for (int b = 0; b < 2; b++) {
                int rc = table_grow(c, c->tab[j], b, std::max<size_t>(cap0, c->tab[j].cap[b]), 0);
                if (rc) return rc;
            }
    int rc = fhh_tree_init(c0);   // fills buffer 0 with the roots (after the growth above)
    if (rc) return rc;
    rc = fhh_tree_init(c1);
    if (rc) return rc;
    S.pair.emplace(c0, c1);
    HIP_TRY(c0, S.ctl.ensure(sizeof(LoopCtl)));
    HIP_TRY(c0, S.sizes.ensure((size_t)levels * (4 + kMaxDims) * 4));
    HIP_TRY(c0, hipMemsetAsync(S.sizes.p, 0, (size_t)levels * (4 + kMaxDims) * 4, c0->stream));
    HIP_TRY(c0, S.ctl_host.ensure(sizeof(LoopCtl)));
    rc = loop_resize(c0, S, cap0, cap0, levels, 0, false, 0, 0, 1);
    if (rc) return rc;
    if (cfg->gc >= 2 && cfg->base_ot) {
        // the OT extensions of every level and chunk each start with 128 Chou–Orlandi base OTs
        // (AlszSender/AlszReceiver::init, collect.rs:454-471): host threads produce them a few levels
        // ahead of this thread's enqueueing, which waits only for the chunk it is about to enqueue
        uint8_t seed[32];
        for (int k = 0; k < 4; k++) {
            const uint64_t z = host_mix64(cfg->prf_seed ^ (0x626173655f6f74ull + (uint64_t)k));
            std::memcpy(seed + 8 * k, &z, 8);
        }
        HIP_TRY(c0, S.base_rk.ensure((size_t)LoopBuffers::kBaseRing * 3 * 128 * 44 * 4));
        S.bot = std::make_unique<BaseOtProducer>(cfg->prf_seed, seed);
        S.base_ot = true;
    }
    if (cfg->probe_n_levels) {
        if (cfg->probe_n_levels > LoopBuffers::kMaxProbe || !cfg->probe_levels || !cfg->probe_n_clients ||
            !cfg->probe_clients || !cfg->probe_seeds || !cfg->probe_ty || !cfg->probe_children)
            return c0->fail(FHH_E_ARG, "sim_crawl: bad probe arguments");
        for (uint32_t i = 0; i < cfg->probe_n_clients; i++)
            if (cfg->probe_clients[i] >= c0->n) return c0->fail(FHH_E_ARG, "sim_crawl: probe client out of range");
        HIP_TRY(c0, S.probe_C.ensure((size_t)cfg->probe_n_levels * 4));
        HIP_TRY(c0, hipMemsetAsync(S.probe_C.p, 0, (size_t)cfg->probe_n_levels * 4, c0->stream));
        HIP_TRY(c0, S.probe_clients.ensure((size_t)cfg->probe_n_clients * 8));
        HIP_TRY(c0, hipMemcpyAsync(S.probe_clients.p, cfg->probe_clients, (size_t)cfg->probe_n_clients * 8,
                                   hipMemcpyHostToDevice, c0->stream));
        HIP_TRY(c0, hipStreamSynchronize(c0->stream));
    }
    uint32_t* l0[kMaxDims] = {nullptr, nullptr, nullptr, nullptr};
    for (uint32_t j = 0; j < d; j++) l0[j] = S.live[0].as<uint32_t>() + (size_t)j * S.E_cap;
    for (uint32_t j = d; j < kMaxDims; j++) l0[j] = l0[0];
    HIP_TRY(c0, launch_loop_init(S.ctl.as<LoopCtl>(), d, (uint32_t)c0->nw, expand_max_group(S.variant),
                                 expand_max_wpi(S.variant),
                                 d, 2, S.grid_waves, S.pos[0].as<uint32_t>(), l0, c0->stream));
    return FHH_OK;
}

// k_expand, both servers, sizes from LoopCtl; then the parity probe's capture of the level's children
int level_expand(Loop& S, const Level& L) {
    fhh_ctx* c0 = S.c0;
    const fhh_sim_config* cfg = S.cfg;
    const uint32_t d = S.d;
    const int par = L.par;
    ExpandLaunch La{};
    La.njobs = 2 * d;
    La.jobs_per_ctx = d;
    La.ctl = S.ctl.as<LoopCtl>();
    for (int s = 0; s < 2; s++)
        for (uint32_t j = 0; j < d; j++) {
            fhh_ctx* c = S.cs[s];
            DimTable& T = c->tab[j];
            ExpandJob& J = La.job[s * d + j];
            J.cw_seed = c->cw_seed.as<uint4>();
            J.cw_bits = c->cw_bits.as<uint64_t>();
            J.src_seed = T.seed[par].as<uint4>();
            J.src_t = T.t[par].as<uint64_t>();
            J.src_y = T.y[par].as<uint64_t>();
            J.dst_seed = T.seed[1 - par].as<uint4>();
            J.dst_t = T.t[1 - par].as<uint64_t>();
            J.dst_y = T.y[1 - par].as<uint64_t>();
            J.live = S.live[par].as<uint32_t>() + (size_t)j * S.E_cap;
            J.level = L.lv;
            J.dim = j;
            J.K = c->K;
            J.npad = (uint32_t)c->npad;
            J.nw = (uint32_t)c->nw;
        }
    size_t slot = 0;
    if (L.timed) HIP_TRY(c0, timing_begin(c0, &slot));
    La.total_items = 1;   // non-zero: the real count comes from LoopCtl
    HIP_TRY(c0, launch_expand(La, S.variant, c0->grid, c0->work_counter.as<uint32_t>(), &c0->expand_seq, c0->stream));
    if (L.timed) HIP_TRY(c0, timing_end(c0, slot, 0));
    c0->stats.expand_launches++;
    for (uint32_t k = 0; k < cfg->probe_n_levels; k++) {
        if (cfg->probe_levels[k] != L.lv) continue;
        const size_t states = (size_t)L.C_cap * cfg->probe_n_clients * d * 2;   // per server
        HIP_TRY(c0, S.probe_seed[k].ensure(2 * states * 16));
        HIP_TRY(c0, S.probe_ty[k].ensure(2 * states));
        S.probe_stride[k] = L.C_cap;
        ProbeArgs pr{};
        for (int s = 0; s < 2; s++)
            for (uint32_t j = 0; j < d; j++) {
                pr.seed[s][j] = S.cs[s]->tab[j].seed[1 - par].as<uint4>();
                pr.t[s][j] = S.cs[s]->tab[j].t[1 - par].as<uint64_t>();
                pr.y[s][j] = S.cs[s]->tab[j].y[1 - par].as<uint64_t>();
            }
        pr.parent_pos = S.pos[par].as<uint32_t>();
        pr.clients = S.probe_clients.as<uint64_t>();
        pr.ctl = S.ctl.as<LoopCtl>();
        pr.out_seed = S.probe_seed[k].as<uint4>();
        pr.out_ty = S.probe_ty[k].as<uint8_t>();
        pr.out_C = S.probe_C.as<uint32_t>() + k;
        pr.C_cap = L.C_cap;
        pr.npad = c0->npad;
        pr.nw = c0->nw;
        pr.n_probe = cfg->probe_n_clients;
        pr.d = d;
        HIP_TRY(c0, launch_probe_states(pr, c0->stream));
    }
    return FHH_OK;
}

// what a level's GC + OT chunks share: set once per level by level_gc_tests
struct GcLevel {
    GtPlan p;
    uint32_t bits;
    uint64_t Gc, tests;     // children per chunk, and their tests
    uint64_t m1, m2;        // OTs per chunk: the labels OT, the share OT
    // the level's two base-OT sessions (OtSender / OtReceiver::init per level and kind,
    // collect.rs:454,460): kind 0 the labels OT, kind 1 the share OT; chunk k extends them
    // from row-PRG block k x (the chunk's blocks), so no two chunks share a pad
    const uint32_t* rk_ot[2];
    uint32_t sw_ot[2][4];
    ChildArgs a;            // the level's children (level_tests)
};

// chunk k's labels OT: the evaluator's labels into gc_evact (row-major), or left in the OT's tile-major Q / T
int chunk_labels_ot(Loop& S, const GcLevel& G, uint64_t k, GcArgs& g) {
    fhh_ctx* c0 = S.c0;
    const GtPlan& p = G.p;
    // 1. the evaluator's input labels by correlated OT (gb_set_fancy_inputs /
    // ev_set_fancy_inputs, equalitytest.rs:67-82,108-119): server 1's choice bits are
    // its share planes [C][bits][nw] from the chunk's first group on, as they stand
    // (m1 a multiple of 128: npad of 64, bits even). The IKNP correlation is the label
    // pair (r05b, OtArgs mode 4): server 0's q_j is the zero label, server 1's t_j =
    // q_j ^ r_j s the active one, with the labels session's s (colour bit set) as the
    // circuit's Delta; server 0's string and mask fold into the circuit
    // (k_gc_garble_cot: no label is drawn, no reply is sent)
    if (!p.tile_major) HIP_TRY(c0, S.gc_evact.ensure(G.m1 * 16));
    for (int c = 0; c < 4; c++) g.delta[c] = G.sw_ot[0][c];
    OtArgs a1{};
    a1.mode = p.tile_major ? 5 : 4;
    a1.rk = G.rk_ot[0];
    for (int c = 0; c < 4; c++) a1.s[c] = G.sw_ot[0][c];
    a1.choices = S.gc_planes[1].as<uint32_t>() + g.g_off * G.bits * p.nw_gc * 2;
    a1.ctr_off = k * ot_session_blocks(G.m1);
    a1.sx = p.tile_major ? nullptr : S.gc_evl.p;
    a1.out = p.tile_major ? nullptr : S.gc_evact.as<uint4>();
    a1.ctl = S.ctl.as<LoopCtl>();
    a1.per_group = p.npad_gc * G.bits;
    a1.g_off = g.g_off;
    a1.ss_k = S.cfg->ot_ss_k;
    int rc = ot_run(c0, a1, G.m1, nullptr);
    if (rc) return rc;
    g.ev_ot = 1;
    if (p.tile_major) {   // the table kernels on the tile-major Q (garbler) / T (evaluator)
        g.lab_tm = 1;
        g.ev_labels = c0->ot_buf[2].as<uint4>();
    }
    return FHH_OK;
}

// one chunk (children [k Gc, (k + 1) Gc)) of a level's tests, a fresh protocol instance: labels OT ->
// garble / evaluate (table or circuit) -> share OT -> the children's sums
int gc_chunk(Loop& S, const Level& L, const GcLevel& G, uint64_t k) {
    fhh_ctx* c0 = S.c0;
    const fhh_sim_config* cfg = S.cfg;
    const GtPlan& p = G.p;
    const uint32_t bits = G.bits, pmode = L.pmode;
    const uint64_t Gc = G.Gc, tests = G.tests, m2 = G.m2;
    uint64_t* part = S.partials.as<uint64_t>();
    const uint64_t g_off = k * Gc;
    fhh_gc_batch gb{};
    gb.groups = Gc;
    gb.clients = (uint32_t)c0->n;
    gb.words = (uint32_t)p.nw_gc;
    gb.bits = bits;
    gc_chunk_material(cfg->prf_seed, L.lv, k, gb.label_key, gb.delta, &gb.mask);
    gb.gate_base = (uint64_t)L.lv << 40;   // the level in the gate tweaks (party_gate_base)
    gb.gb_planes_dev = S.gc_planes[0].as<uint64_t>();
    gb.ev_planes_dev = S.gc_planes[1].as<uint64_t>();
    gb.tables_dev = S.gc_tables.as<uint8_t>();
    gb.gb_labels_dev = S.gc_gbl.as<uint8_t>();
    gb.ev_labels_dev = S.gc_evl.as<uint8_t>();
    gb.decode_dev = S.gc_decode.as<uint8_t>();
    gb.out_dev = S.gc_out.as<uint8_t>();
    GcArgs g{};
    int rc = gc_args(c0, &gb, g);
    if (rc) return rc;
    g.ctl = S.ctl.as<LoopCtl>();
    g.g_off = g_off;
    if (p.real_ot && (rc = chunk_labels_ot(S, G, k, g))) return rc;
    // r05c: at the FE levels the share comes from the circuit's output labels (W_0 and
    // W_0 ^ Delta of o = eq ^ mask in the share C-OT's roles): server 0's node value r1 and
    // the 8-B y from k_gc_garble_cot, server 1's value from k_gc_eval — no second OT.
    // r05d: the table's tests (GtPlan::table) take the share from ONE garbled table per test
    if (p.table) {
        // r06 (tile-major table): the kernels add the node values per child into the level's
        // partials themselves (no stored values, no k_child_sums_fe pass)
        const bool fused = p.fused_sums;
        if (!fused) for (int sv = 0; sv < 2; sv++) HIP_TRY(c0, S.gc_val[sv].ensure(tests * 8));
        HIP_TRY(c0, S.gc_msgs.ensure(tests * (((size_t)1 << bits) - 1) * 8));
        g.gt_msgs = S.gc_msgs.as<uint64_t>();
        g.node_partials = fused ? part : nullptr;
        g.node_off = 0;
        g.ring32 = p.ring32 ? 1u : 0u;   // (row-major: u32 values [tests] in gc_val, u32 messages)
        g.sh_gb = fused ? nullptr : S.gc_val[0].as<uint64_t>();
        HIP_TRY(c0, launch_gt_garble(g, c0->stream, c0->protocol_grid));
        g.ev_labels = p.tile_major ? c0->ot_buf[0].as<uint4>() : S.gc_evact.as<uint4>();
        g.sh_gb = nullptr;
        g.sh_ev = fused ? nullptr : S.gc_val[1].as<uint64_t>();
        HIP_TRY(c0, launch_gt_eval(g, c0->stream, c0->protocol_grid));
        if (p.ring32 && !fused)   // the row-major Z_2^32 values into the partials' low sums
            for (uint32_t sv = 0; sv < 2; sv++)
                HIP_TRY(c0, launch_ring32_child_partials(S.gc_val[sv].as<uint32_t>(), c0->n, Gc,
                                                         S.ctl.as<LoopCtl>(), g_off, part, 2 * sv,
                                                         c0->stream));
    } else if (p.lshare) {
        for (int sv = 0; sv < 2; sv++) HIP_TRY(c0, S.gc_val[sv].ensure(tests * 8));
        HIP_TRY(c0, S.gc_y.ensure(tests * 8));
        g.sh_gb = S.gc_val[0].as<uint64_t>();
        g.sh_y = S.gc_y.as<uint64_t>();
    }
    if (!p.table) {
        HIP_TRY(c0, launch_gc_garble(g, c0->stream, c0->protocol_grid));
        if (p.real_ot) {
            g.ev_labels = S.gc_evact.as<uint4>();
            g.sh_gb = nullptr;
            if (p.lshare) {
                g.sh_ev = S.gc_val[1].as<uint64_t>();
            } else {
                // k_gc_eval ballot-packs its outputs as the share-conversion OT's choice words
                uint32_t* och = nullptr;
                HIP_TRY(c0, ot_choices_buffer(c0, m2, &och));
                g.out_packed = och;
                g.out_dup = p.per2;
            }
        }
        HIP_TRY(c0, launch_gc_eval(g, c0->stream, c0->protocol_grid));
    }
    ChildArgs ca = G.a;   // this chunk's children
    ca.c_off = g_off;
    ca.c_cnt = Gc;
    ca.gc_out = g.out;
    ca.gc_N = g.N;
    ca.gc_mask = g.mask;
    if (p.real_ot && !p.lshare) {
        // 2. the share conversion by correlated OT (collect.rs:846-876 at the last level,
        // where a FieldElm travels as a BlockPair = 2 OTs): server 0's pair is
        // (H(q_j), H(q_j) +- 1) ordered by its mask, its node value r1 = H(q_j) + mask;
        // server 1 chooses with its GC output bit
        const size_t vb = pmode == 1 ? 8 : 16;
        for (int sv = 0; sv < 2; sv++) HIP_TRY(c0, S.gc_val[sv].ensure(m2 * vb));
        OtArgs a2{};
        a2.mode = pmode == 1 ? 2 : 3;
        a2.mask = g.mask;
        a2.rk = G.rk_ot[1];
        for (int c = 0; c < 4; c++) a2.s[c] = G.sw_ot[1][c];
        a2.choices = g.out_packed;
        a2.ctr_off = k * ot_session_blocks(m2);
        a2.sx = S.gc_val[0].p;
        a2.out = S.gc_val[1].as<uint4>();
        a2.ctl = S.ctl.as<LoopCtl>();
        a2.per_group = (uint64_t)c0->n * p.per2;
        a2.g_off = g_off;
        a2.ss_k = cfg->ot_ss_k;
        rc = ot_run(c0, a2, m2, nullptr);
        if (rc) return rc;
    }
    if (p.real_ot) {   // both servers' node values: the label shares' or the share OT's
        ca.ot_val[0] = S.gc_val[0].p;
        ca.ot_val[1] = S.gc_val[1].p;
    }
    // the chunk's children's sums (FE: atomics into the partials k_prune zeroed;
    // FE255: one store per child)
    if (pmode == 1) {
        if (!p.fused_sums && !p.ring32) HIP_TRY(c0, launch_child_sums_fe(ca, part, c0->stream, false));
    } else {
        HIP_TRY(c0, launch_child_sums_fe255(ca, part, c0->stream));
    }
    return FHH_OK;
}

// garbled-circuit equality (tree_crawl with gc_sender, collect.rs:419-482): both
// servers' share planes, server 0 garbles, server 1 evaluates. The level's tests
// run in chunks of Gc children (bounded memory at 1M clients; the reference
// splits a level's tests over its channels the same way, collect.rs:423-430), each
// chunk a fresh protocol instance: its own garbler key / Delta / mask, and its own
// row-PRG range of the level's base-OT sessions. What does not depend on the chunk is done here:
// the planes, the base-OT requests and uploads, the buffers
int level_gc_tests(Loop& S, const Level& L, const ChildArgs& a) {
    fhh_ctx* c0 = S.c0;
    const fhh_sim_config* cfg = S.cfg;
    GcLevel G{};
    G.p = S.plan(L.pmode);
    G.a = a;
    const GtPlan& p = G.p;
    const uint32_t bits = G.bits = 2 * S.d;
    const size_t plane_bytes = (size_t)L.C_cap * bits * p.nw_gc * 8;
    for (int s = 0; s < 2; s++) HIP_TRY(c0, S.gc_planes[s].ensure(plane_bytes));
    size_t gc_slot = 0;
    if (L.timed) HIP_TRY(c0, timing_begin(c0, &gc_slot));
    ChildArgs pa = a;
    pa.plane_nw = (uint32_t)p.nw_gc;
    HIP_TRY(c0, launch_share_planes(pa, S.gc_planes[0].as<uint64_t>(), c0->stream));
    pa.s0 = a.s1;
    HIP_TRY(c0, launch_share_planes(pa, S.gc_planes[1].as<uint64_t>(), c0->stream));
    const uint64_t Gc = G.Gc = std::min<uint64_t>(
        L.C_cap, std::max<uint64_t>(1, S.gc_budget / (p.bytes_per_test * std::max<uint64_t>(c0->npad, 1))));
    const uint64_t chunks = (L.C_cap + Gc - 1) / Gc;
    const uint64_t tests = G.tests = Gc * c0->n;
    const uint64_t m1 = G.m1 = Gc * bits * p.npad_gc;
    G.m2 = tests * p.per2;
    if (p.real_ot) {
        HIP_TRY(c0, c0->ot_rk.ensure((size_t)2 * 3 * 128 * 44 * 4));
        if (S.base_ot) {
            // keep the producer well ahead of the enqueueing: the first levels take ~1 ms of
            // GPU time against ~9 ms per CO15 instance, so at 4 levels ahead the loop waited
            // 0.56-0.59 s per 1M crawl (base_ot_stall_ms); 32 levels = 64 instances, 4.3 MB
            // (kind 1, the share OT, runs at the FieldElm level only: the FE levels take their
            // share from the circuit's output labels, r05c)
            constexpr uint32_t kAhead = 32;
            for (uint32_t l = L.lv; l < std::min(S.levels, L.lv + kAhead); l++)
                for (uint32_t w = 0; w < (l + 1 == S.levels ? 2u : 1u); w++) (void)S.bot->request(l, w);
        }
        for (uint32_t w = 0; w < (L.pmode == 2 ? 2u : 1u); w++) {
            ot_level_choice(cfg->prf_seed, L.lv, w, G.sw_ot[w]);
            if (S.base_ot) {
                int rc = upload_base_ot(c0, S, L.lv, w, &G.rk_ot[w]);
                if (rc) return rc;
            } else {
                uint32_t* rk = c0->ot_rk.as<uint32_t>() + (size_t)w * 3 * 128 * 44;
                HIP_TRY(c0, launch_ot_level_keys(cfg->prf_seed, L.lv, w, G.sw_ot[w], rk, c0->stream));
                G.rk_ot[w] = rk;
            }
        }
    }
    // (the garbled table writes no half-gate tables, decoding bits or output bytes)
    HIP_TRY(c0, S.gc_tables.ensure(p.table ? 16 : (size_t)std::max(bits - 1, 1u) * 2 * tests * 16));
    // garbler labels: the ideal-OT garbler's only (the r05 garbler folds its string in)
    HIP_TRY(c0, S.gc_gbl.ensure(p.real_ot ? 16 : (size_t)(bits + 1) * tests * 16));
    // ideal OT: the evaluator's active labels [bits][tests]; OT mode: its zero labels (the
    // labels C-OT's sender messages) at OT index (g bits + j) npad + i (r06 tile-major table: none,
    // the kernels read Q / T)
    HIP_TRY(c0, S.gc_evl.ensure(p.windows ? 16
                                          : std::max<size_t>((size_t)bits * tests, p.real_ot && !p.tile_major ? m1 : 0) * 16));
    HIP_TRY(c0, S.gc_decode.ensure(p.table ? 1 : tests));
    HIP_TRY(c0, S.gc_out.ensure(p.table ? 1 : tests));
    for (uint64_t k = 0; k < chunks; k++) {
        int rc = gc_chunk(S, L, G, k);
        if (rc) return rc;
    }
    if (L.timed) HIP_TRY(c0, timing_end(c0, gc_slot, kGcotTag));
    return FHH_OK;
}

// equality count / simulated OT sums per child, or the GC + OT protocol (cfg->gc)
int level_tests(Loop& S, const Level& L) {
    fhh_ctx *c0 = S.c0, *c1 = S.c1;
    const int par = L.par;
    ChildArgs a{};
    for (uint32_t j = 0; j < S.d; j++) {
        a.s0.t[j] = c0->tab[j].t[1 - par].as<uint64_t>();
        a.s0.y[j] = c0->tab[j].y[1 - par].as<uint64_t>();
        a.s1.t[j] = c1->tab[j].t[1 - par].as<uint64_t>();
        a.s1.y[j] = c1->tab[j].y[1 - par].as<uint64_t>();
    }
    a.parent_pos = S.pos[par].as<uint32_t>();
    a.valid = c0->valid.as<uint64_t>();
    a.C = L.C_cap;   // grid hint; the real C comes from LoopCtl
    a.d = S.d;
    a.nw = (uint32_t)c0->nw;
    a.client_base = c0->client_base;
    a.prf_seed = S.cfg->prf_seed;
    a.level = L.lv;
    a.n = (uint32_t)c0->n;
    a.ctl = S.ctl.as<LoopCtl>();
    uint64_t* part = S.partials.as<uint64_t>();
    if (S.cfg->gc && L.pmode != 0) return level_gc_tests(S, L, a);
    if (L.pmode == 0) {
        HIP_TRY(c0, launch_eq_count(a, part, c0->stream));
    } else if (L.pmode == 1) {
        HIP_TRY(c0, launch_child_sums_fe(a, part, c0->stream, false));
    } else {
        HIP_TRY(c0, launch_child_sums_fe255(a, part, c0->stream));
    }
    return FHH_OK;
}

// cross-rank sum (client-sharded multi-GPU), and the level's record for cfg->counts
int level_reduce(Loop& S, const Level& L) {
    fhh_ctx* c0 = S.c0;
    const fhh_sim_config* cfg = S.cfg;
    // (the count is the capacity bound: entries past C are never read)
    const uint64_t count = L.C_cap * L.per;
    if (S.distributed) {
        const bool timed = L.timed && cfg->comm;   // (the callback path drains the stream: nothing to time)
        size_t ar_slot = 0;
        if (timed) HIP_TRY(c0, timing_begin(c0, &ar_slot));
        int rc = loop_allreduce(S, S.partials.as<uint64_t>(), S.red(), count);
        if (rc) return rc;
        if (timed) HIP_TRY(c0, timing_end(c0, ar_slot, kAllreduceTag));
    }
    if (S.record) {
        const size_t off = S.rec_off.empty() ? 0 : S.rec_off.back() + (size_t)S.rec_stride.back();
        const size_t need = (off + count) * 8;
        if (S.rec.bytes < need) {
            PinnedBuf nb;
            HIP_TRY(c0, hipStreamSynchronize(c0->stream));
            HIP_TRY(c0, nb.ensure(std::max(need * 2, (size_t)1 << 20)));
            if (S.rec.p) std::memcpy(nb.p, S.rec.p, S.rec.bytes);
            S.rec.swap(nb);
        }
        S.rec_off.resize(L.lv + 1);
        S.rec_stride.resize(L.lv + 1);
        S.rec_off[L.lv] = off;
        S.rec_stride[L.lv] = (uint32_t)count;   // u64 words recorded for this level
        // mode 0: counts; FE: the 4 limbs; FE255: the 16 limbs (v0 - v1 derived at the end)
        HIP_TRY(c0, hipMemcpyAsync(S.rec.as<uint64_t>() + off, S.red(), (size_t)count * 8, hipMemcpyDeviceToHost, c0->stream));
    }
    return FHH_OK;
}

// leader keep decision + prune (or final list at the last level)
int level_prune(Loop& S, const Level& L) {
    fhh_ctx* c0 = S.c0;
    const uint32_t d = S.d;
    if (L.last) HIP_TRY(c0, S.final_vals.ensure((size_t)S.F_cap * 20 * 4));
    PruneArgs pa{};
    pa.ctl = S.ctl.as<LoopCtl>();
    pa.partials = S.red();
    pa.mode = L.pmode;
    pa.d = d;
    pa.thr = S.thr;
    pa.thr_last = S.thr_last;
    pa.last = L.last ? 1 : 0;
    pa.pos_in = S.pos[L.par].as<uint32_t>();
    pa.pos_out = S.pos[1 - L.par].as<uint32_t>();
    for (uint32_t j = 0; j < kMaxDims; j++)
        pa.live_out[j] = S.live[1 - L.par].as<uint32_t>() + (size_t)std::min(j, d - 1) * S.E_cap;
    pa.mark = S.mark.as<uint32_t>();
    pa.hist_out = S.hist_ptr[L.lv];
    pa.sizes_out = S.sizes.as<uint32_t>() + (size_t)L.lv * (4 + kMaxDims);
    pa.final_vals = L.last ? S.final_vals.as<uint32_t>() : nullptr;
    pa.E_cap = S.E_cap;
    pa.F_cap = S.F_cap;
    pa.level = L.lv;
    pa.nw = (uint32_t)c0->nw;
    pa.njobs_per_ctx = d;
    pa.nctx = 2;
    pa.grid_waves = S.grid_waves;
    pa.unit = (uint32_t)c0->nw;
    pa.max_group = expand_max_group(S.variant);
    pa.max_wpi = expand_max_wpi(S.variant);
    pa.zero_partials = (S.cfg->mode != 0 && !L.last) ? S.partials.as<uint64_t>() : nullptr;
    pa.ring32 = S.plan(L.pmode).ring32 ? 1u : 0u;
    pa.zero_count = (uint64_t)L.C_cap * 4;
    HIP_TRY(c0, launch_prune(pa, c0->stream));
    return FHH_OK;
}

// a batch ended in an abort (h, read back at level batch_end): grow, keep what the prune of
// h->abort_level reads; the caller resumes there
int loop_grow(Loop& S, const LoopCtl* h, uint32_t batch_end) {
    fhh_ctx* c0 = S.c0;
    const uint32_t d = S.d;
    const uint32_t la = h->abort_level;
    const bool la_last = la + 1 == S.levels;
    // an abort at the last level lacks room for the final nodes only: nothing is expanded after it, and the
    // tables of parity la & 1 and the live lists of that parity are the frontier the crawl leaves to the engine
    // (loop_readback), so the tables stay as they are and the lists are carried over
    uint32_t nE = S.E_cap;
    int rc = la_last ? FHH_OK : loop_entry_cap(S, std::max<uint32_t>(h->need_entries, 1), la, nE);
    if (rc) return rc;
    const uint32_t nF = std::max(S.F_cap, next_pow2(std::max<uint32_t>(h->need_nodes, 1)) * 2);
    const uint32_t la_per = S.cfg->mode == 0 ? 1 : (la_last ? 16 : 4);
    if (std::getenv("FHH_DEBUG_LOOP"))
        std::fprintf(stderr, "[fhh loop] abort at level %u (batch end %u): need_entries %u need_nodes %u "
                     "F %u C %u -> E_cap %u F_cap %u\n", la, batch_end, h->need_entries, h->need_nodes, h->F,
                     h->C, nE, nF);
    // the tables of parity la & 1 are rewritten by level la + 1: released first, so the
    // peak while the preserved ones are copied is one old table, not all of them
    for (fhh_ctx* c : S.cs)
        for (uint32_t j = 0; j < d && !la_last; j++) table_release(c->tab[j], la & 1);
    for (fhh_ctx* c : S.cs)
        for (uint32_t j = 0; j < d && !la_last; j++) {
            // child tables of level la (parity 1 - la&1) hold 2 * n_live(la) entries
            rc = table_grow(c, c->tab[j], 1 - (la & 1), nE, 2 * (size_t)h->n_live[j]);
            if (rc) return rc;
        }
    for (fhh_ctx* c : S.cs)
        for (uint32_t j = 0; j < d && !la_last; j++) {
            rc = table_grow(c, c->tab[j], la & 1, nE, 0);
            if (rc) return rc;
        }
    rc = loop_resize(c0, S, nE, nF, S.levels, la, true, h->F, h->C, la_per, la_last ? h->n_live : nullptr);
    if (rc) return rc;
    const uint32_t zero = 0;
    HIP_TRY(c0, hipMemcpy(S.ctl.p, &zero, 4, hipMemcpyHostToDevice));   // abort = 0
    return FHH_OK;
}

// readback: sizes, hist, final values, frontier -> host-side state and stats of both servers; sz = the
// levels' size rows [levels][4 + kMaxDims] (C, kept, -, -, n_live per dim)
int loop_readback(Loop& S, std::vector<uint32_t>& sz) {
    fhh_ctx* c0 = S.c0;
    const fhh_sim_config* cfg = S.cfg;
    const uint32_t d = S.d, levels = S.levels;
    // every level's hist row is packed on the device (k_gather_hist) and copied in one transfer
    const uint64_t hist_cap = (uint64_t)levels * S.F_cap;
    HIP_TRY(c0, S.hist_rows.ensure((size_t)levels * sizeof(uint32_t*)));
    HIP_TRY(c0, S.hist_packed.ensure(hist_cap * 4));
    HIP_TRY(c0, hipMemcpyAsync(S.hist_rows.p, S.hist_ptr.data(), (size_t)levels * sizeof(uint32_t*),
                               hipMemcpyHostToDevice, c0->stream));
    HIP_TRY(c0, launch_gather_hist(S.sizes.as<uint32_t>(), 4 + kMaxDims, S.hist_rows.as<const uint32_t*>(), levels,
                                   S.hist_packed.as<uint32_t>(), hist_cap, c0->stream));
    // (the engine stream is non-blocking: plain hipMemcpy would not wait for k_gather_hist)
    sz.resize((size_t)levels * (4 + kMaxDims));
    HIP_TRY(c0, hipMemcpyAsync(sz.data(), S.sizes.p, sz.size() * 4, hipMemcpyDeviceToHost, c0->stream));
    HIP_TRY(c0, hipStreamSynchronize(c0->stream));
    uint64_t hist_total = 0;
    for (uint32_t lv = 0; lv < levels; lv++) hist_total += sz[(size_t)lv * (4 + kMaxDims) + 1];
    if (hist_total > hist_cap) return c0->fail(FHH_E_STATE, "loop: kept-children lists exceed their capacity");
    std::vector<uint32_t> packed(hist_total);
    if (hist_total) {
        HIP_TRY(c0, hipMemcpyAsync(packed.data(), S.hist_packed.p, hist_total * 4, hipMemcpyDeviceToHost, c0->stream));
        HIP_TRY(c0, hipStreamSynchronize(c0->stream));
    }
    std::vector<std::vector<std::pair<uint32_t, uint32_t>>> hist(levels);
    const uint32_t mask = (1u << d) - 1;
    for (uint32_t lv = 0, off = 0; lv < levels; lv++) {
        const uint32_t nf = sz[(size_t)lv * (4 + kMaxDims) + 1];
        hist[lv].reserve(nf);
        for (uint32_t k = 0; k < nf; k++) hist[lv].emplace_back(packed[off + k] >> d, packed[off + k] & mask);
        off += nf;
    }
    const uint32_t nfin = sz[(size_t)(levels - 1) * (4 + kMaxDims) + 1];
    std::vector<uint32_t> fv((size_t)nfin * 20);
    if (nfin) HIP_TRY(c0, hipMemcpy(fv.data(), S.final_vals.p, fv.size() * 4, hipMemcpyDeviceToHost));
    // frontier before the last crawl: depth levels-1, states in table buffer (levels-1)&1
    const int fpar = (levels - 1) & 1;
    const uint32_t Ffront = levels >= 2 ? sz[(size_t)(levels - 2) * (4 + kMaxDims) + 1] : 1;
    std::vector<uint32_t> fpos((size_t)Ffront * d);
    if (Ffront) HIP_TRY(c0, hipMemcpy(fpos.data(), S.pos[fpar].p, fpos.size() * 4, hipMemcpyDeviceToHost));
    std::vector<std::vector<uint32_t>> flive(d);
    for (uint32_t j = 0; j < d; j++) {
        const uint32_t nl = levels >= 2 ? sz[(size_t)(levels - 2) * (4 + kMaxDims) + 4 + j] : 1;
        flive[j].resize(nl);
        if (nl)
            HIP_TRY(c0, hipMemcpy(flive[j].data(), S.live[fpar].as<uint32_t>() + (size_t)j * S.E_cap, (size_t)nl * 4,
                                  hipMemcpyDeviceToHost));
    }
    // entries k_expand read per level: the dims' live entries of the level before (the roots at level 0)
    std::vector<uint64_t> live_sum(levels, 0);
    for (uint32_t lv = 0; lv < levels; lv++)
        for (uint32_t j = 0; j < d; j++) live_sum[lv] += lv == 0 ? 1 : sz[(size_t)(lv - 1) * (4 + kMaxDims) + 4 + j];
    for (int s = 0; s < 2; s++) {
        fhh_ctx* c = S.cs[s];
        c->hist.assign(hist.begin(), hist.begin() + (levels - 1));
        c->last_hist = c->hist;
        c->last_depth = levels;
        c->last_nodes = hist[levels - 1];
        c->last_values.assign(nfin, Limbs10{});
        for (uint32_t k = 0; k < nfin; k++) {
            if (cfg->mode == 0 && s == 1) continue;   // count mode: values on server 0 (host loop convention)
            std::memcpy(c->last_values[k].data(), &fv[(size_t)k * 20 + (cfg->mode == 0 ? 0 : 10 * s)], 40);
        }
        c->frontier.assign(Ffront, Node{});
        for (uint32_t k = 0; k < Ffront; k++)
            for (uint32_t j = 0; j < d; j++) c->frontier[k].pos[j] = fpos[(size_t)k * d + j];
        for (uint32_t j = 0; j < d; j++) {
            c->tab[j].live = flive[j];
            c->tab[j].cur = fpar;
            c->child_buf[j] = 1 - fpar;
        }
        c->level = levels - 1;
        c->pending_C = 0;
        c->phase = Phase::kFrontier;   // after tree_prune_last (collect.rs:931-942)
        for (uint32_t lv = 0; lv < levels; lv++) {
            c->stats.aes_blocks += live_sum[lv] * 4 * c->n;
            c->stats.ref_evals += (uint64_t)sz[(size_t)lv * (4 + kMaxDims)] * c->n * 2 * d;
            c->stats.levels += 1;
        }
    }
    // expand_blocks_timed for c0's timed launches: both servers
    for (uint32_t lv = 0; lv < levels && c0->timing; lv++)
        if (lv % c0->timing_every == 0) c0->stats.expand_blocks_timed += live_sum[lv] * 4 * c0->n * 2;
    return FHH_OK;
}

// optional per-level records: cfg->level_children / level_kept / counts
void loop_records(const Loop& S, const std::vector<uint32_t>& sz) {
    const fhh_sim_config* cfg = S.cfg;
    const bool ring32 = S.plan(1).ring32;   // r06: the FE levels' shares are Z_2^32's
    uint64_t off = 0;
    for (uint32_t lv = 0; lv < S.levels; lv++) {
        const uint32_t C = sz[(size_t)lv * (4 + kMaxDims)];
        if (cfg->level_children) cfg->level_children[lv] = C;
        if (cfg->level_kept) cfg->level_kept[lv] = sz[(size_t)lv * (4 + kMaxDims) + 1];
        if (S.record && lv < S.rec_off.size()) {
            const uint64_t* r = S.rec.as<uint64_t>() + S.rec_off[lv];
            const bool lvl_last = lv + 1 == S.levels;
            for (uint32_t c = 0; c < C && off + c < cfg->counts_capacity; c++) {
                uint64_t v;
                if (cfg->mode == 0) {
                    v = r[c];
                } else if (!lvl_last && ring32) {
                    v = (uint32_t)(r[c * 4] - r[c * 4 + 2]);
                } else if (!lvl_last) {
                    v = fe_sub_canon(fe_canon_from_limbs(r[c * 4], r[c * 4 + 1]), fe_canon_from_limbs(r[c * 4 + 2], r[c * 4 + 3]));
                } else {
                    const auto dv = fe255_sub(fe255_reduce(limbs_from_partials(r + (size_t)c * 16)),
                                              fe255_reduce(limbs_from_partials(r + (size_t)c * 16 + 8)));
                    v = (uint64_t)dv[0] | ((uint64_t)dv[1] << 32);
                }
                cfg->counts[off + c] = v;
            }
        }
        off += C;
    }
}

// the parity probe's captured states -> cfg->probe_children / probe_seeds / probe_ty
int loop_probe_readback(Loop& S) {
    fhh_ctx* c0 = S.c0;
    const fhh_sim_config* cfg = S.cfg;
    if (!cfg->probe_n_levels) return FHH_OK;
    std::vector<uint32_t> pC(cfg->probe_n_levels);
    HIP_TRY(c0, hipMemcpy(pC.data(), S.probe_C.p, pC.size() * 4, hipMemcpyDeviceToHost));
    const size_t row = (size_t)cfg->probe_n_clients * S.d * 2;   // states per (server, child)
    const size_t cap = cfg->probe_capacity;
    for (uint32_t k = 0; k < cfg->probe_n_levels; k++) {
        cfg->probe_children[k] = pC[k];
        const size_t nc = std::min<size_t>(std::min<size_t>(pC[k], cap), S.probe_stride[k]);
        if (!nc || !S.probe_seed[k].p) continue;
        for (int s = 0; s < 2; s++) {
            uint8_t* hs = cfg->probe_seeds + (((size_t)k * 2 + s) * cap) * row * 16;
            uint8_t* ht = cfg->probe_ty + (((size_t)k * 2 + s) * cap) * row;
            HIP_TRY(c0, hipMemcpy(hs, S.probe_seed[k].as<uint8_t>() + (size_t)s * S.probe_stride[k] * row * 16,
                                  nc * row * 16, hipMemcpyDeviceToHost));
            HIP_TRY(c0, hipMemcpy(ht, S.probe_ty[k].as<uint8_t>() + (size_t)s * S.probe_stride[k] * row, nc * row,
                                  hipMemcpyDeviceToHost));
        }
    }
    return FHH_OK;
}

// The whole crawl enqueued without host round trips: every kBatch levels (and at the end) LoopCtl comes
// back; after an abort the buffers grow and the crawl resumes at the prune of the level that aborted.
int sim_crawl_device_loop(fhh_ctx* c0, fhh_ctx* c1, const fhh_sim_config* cfg, uint32_t levels, uint64_t thr,
                          uint32_t thr_last) {
    PhaseClock pc;
    Loop S(c0, c1, cfg, levels, thr, thr_last);
    int rc = loop_setup(S);
    if (rc) return rc;
    pc.mark("setup");
    const uint32_t kBatch = 32;
    bool prune_only = false;           // resume after growth: prune of this level only
    for (uint32_t lv = 0; lv < levels;) {
        const Level L(S, lv);
        if (!prune_only) {
            if ((rc = level_expand(S, L)) || (rc = level_tests(S, L)) || (rc = level_reduce(S, L))) return rc;
        }
        prune_only = false;
        rc = level_prune(S, L);
        if (rc) return rc;
        lv++;
        if (lv % kBatch == 0 || lv == levels) {
            HIP_TRY(c0, hipMemcpyAsync(S.ctl_host.p, S.ctl.p, sizeof(LoopCtl), hipMemcpyDeviceToHost, c0->stream));
            rc = ctx_sync(c0);
            if (rc) return rc;
            const LoopCtl* h = S.ctl_host.as<LoopCtl>();
            if (h->abort) {
                rc = loop_grow(S, h, lv);
                if (rc) return rc;
                lv = h->abort_level;
                prune_only = true;
            }
        }
    }
    if (S.bot) {
        // every instance the crawl used was waited for at its upload; lookahead ones still running
        // are abandoned (the destructor stops the workers after their current instance)
        std::lock_guard<std::mutex> lk(S.bot->mu);
        c0->stats.base_ot_ms += S.bot->compute_ms;
        c0->stats.base_ot_stall_ms += S.bot->stall_ms;
        c0->stats.base_ot_instances += S.bot->computed;
    }
    c0->loop_cap_hint = std::max(S.E_cap, S.F_cap);   // the next crawl starts at this size
    pc.mark("loop");
    std::vector<uint32_t> sz;
    rc = loop_readback(S, sz);
    if (rc) return rc;
    loop_records(S, sz);
    rc = loop_probe_readback(S);
    if (rc) return rc;
    pc.mark("readback");
    return FHH_OK;
}

extern "C" {

int fhh_sim_eq_count(fhh_ctx* c0, fhh_ctx* c1, uint64_t* counts) {
    if (!c0 || !c1) {
        g_err = "null fhh_ctx";
        return FHH_E_ARG;
    }
    if (c0->group || c1->group) return c0->fail(FHH_E_ARG, "sim_eq_count: per-shard harness entry (use fhh_sim_crawl on a multi-device ctx)");
    int rc = ctx_set_device(c0);
    if (rc) return rc;
    if (!counts) return c0->fail(FHH_E_ARG, "sim_eq_count: NULL counts");
    return sim_eq_count_impl(c0, c1, nullptr, counts);
}

int fhh_sim_ot_sums(fhh_ctx* c0, fhh_ctx* c1, uint64_t prf_seed, void* sums0, void* sums1) {
    if (!c0 || !c1) {
        g_err = "null fhh_ctx";
        return FHH_E_ARG;
    }
    if (c0->group || c1->group) return c0->fail(FHH_E_ARG, "sim_ot_sums: per-shard harness entry (use fhh_sim_crawl on a multi-device ctx)");
    int rc = ctx_set_device(c0);
    if (rc) return rc;
    if (!sums0 || !sums1) return c0->fail(FHH_E_ARG, "sim_ot_sums: NULL buffer");
    return sim_ot_sums_impl(c0, c1, nullptr, prf_seed, sums0, sums1);
}

int fhh_sim_crawl(fhh_ctx* c0, fhh_ctx* c1, const fhh_sim_config* cfg) {
    if (!c0 || !c1 || !cfg) {
        g_err = "sim_crawl: NULL argument";
        return FHH_E_ARG;
    }
    if (c0->group || c1->group) return group_sim_crawl(c0, c1, cfg);
    int rc = ctx_set_device(c0);
    if (rc) return rc;
    const uint32_t levels = cfg->levels ? cfg->levels : c0->L;
    if (levels > c0->L) return c0->fail(FHH_E_ARG, "sim_crawl: levels > data_len");
    if (cfg->mode > 1) return c0->fail(FHH_E_ARG, "sim_crawl: bad mode");
    if (cfg->gc > 3)
        return c0->fail(FHH_E_ARG, "sim_crawl: gc must be 0, 1 (ideal OT), 2 (OT extension) or 3 (2 with the circuit at every level)");
    if (cfg->gc && (cfg->mode != 1 || cfg->host_loop))
        return c0->fail(FHH_E_ARG, "sim_crawl: gc needs mode 1 (OT share values) and the device loop");
    if (cfg->gc && 2 * c0->d > (uint32_t)kGcMaxBits) return c0->fail(FHH_E_ARG, "sim_crawl: gc supports d <= 4");
    if (cfg->ot_ss_k > 1 && cfg->ot_ss_k != 2 && cfg->ot_ss_k != 4)
        return c0->fail(FHH_E_ARG, "sim_crawl: ot_ss_k must be 0 / 1 (IKNP), 2 or 4 (SoftSpoken)");
    if (cfg->probe_n_levels && cfg->host_loop)
        return c0->fail(FHH_E_ARG, "sim_crawl: the probe instruments the device loop (host_loop = 0)");
    if (c0->device != c1->device) return c0->fail(FHH_E_ARG, "sim_crawl: ctxs on different devices");
    if (c0->d != c1->d || c0->L != c1->L) return c0->fail(FHH_E_ARG, "sim_crawl: ctx shapes differ");
    // leader.rs:193-194 and 245-246
    const uint64_t thr = std::max<uint64_t>(1, (uint64_t)(cfg->threshold * (double)cfg->nclients_total));
    // `as u32` in Rust saturates (leader.rs:245): clamp before narrowing
    const double thr_last_f = cfg->threshold * (double)cfg->nclients_total;
    const uint32_t thr_last =
        std::max<uint32_t>(1, thr_last_f >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)(uint64_t)thr_last_f);
    if (!cfg->host_loop) {
        PhaseClock total;
        rc = sim_crawl_device_loop(c0, c1, cfg, levels, thr, thr_last);   // incl. buffer teardown
        total.mark("total");
        return rc;
    }
    rc = fhh_tree_init(c0);
    if (rc) return rc;
    rc = fhh_tree_init(c1);
    if (rc) return rc;
    PairScope pair(c0, c1);
    uint64_t counts_off = 0;
    std::vector<uint64_t> vals, s0, s1;
    std::vector<uint32_t> l0, l1;
    std::vector<uint8_t> keep;
    for (uint32_t lv = 0; lv < levels; lv++) {
        const bool last = lv + 1 == levels;
        rc = crawl_pair(c0, c1, last);
        if (rc) return rc;
        const uint64_t C = c0->pending_C;
        keep.assign(C, 0);
        if (cfg->mode == 0) {
            vals.resize(C);
            rc = sim_eq_count_impl(c0, c1, cfg, vals.data());
            if (rc) return rc;
            for (uint64_t c = 0; c < C; c++) keep[c] = vals[c] >= (last ? (uint64_t)thr_last : thr);
            if (cfg->counts && counts_off + C <= cfg->counts_capacity)
                std::memcpy(cfg->counts + counts_off, vals.data(), C * 8);
            counts_off += C;
            if (last) {
                for (uint64_t c = 0; c < C; c++) {
                    Limbs10 v{};
                    v[0] = (uint32_t)vals[c];
                    v[1] = (uint32_t)(vals[c] >> 32);
                    c0->last_values[c] = v;
                    c1->last_values[c] = Limbs10{};
                }
            }
        } else if (!last) {
            s0.resize(C);
            s1.resize(C);
            rc = sim_ot_sums_impl(c0, c1, cfg, cfg->prf_seed, s0.data(), s1.data());
            if (rc) return rc;
            rc = fhh_keep_values(thr, s0.data(), s1.data(), C, keep.data());
            if (rc) return rc;
            if (cfg->counts && counts_off + C <= cfg->counts_capacity)
                for (uint64_t c = 0; c < C; c++)
                    cfg->counts[counts_off + c] = s0[c] >= s1[c] ? s0[c] - s1[c] : s0[c] + (kFeP - s1[c]);
            counts_off += C;
        } else {
            l0.resize(C * 10);
            l1.resize(C * 10);
            rc = sim_ot_sums_impl(c0, c1, cfg, cfg->prf_seed, l0.data(), l1.data());
            if (rc) return rc;
            rc = fhh_keep_values_last(thr_last, l0.data(), l1.data(), C, keep.data());
            if (rc) return rc;
            if (cfg->counts && counts_off + C <= cfg->counts_capacity) {
                std::vector<uint32_t> fv(C * 8);
                fhh_final_values(l0.data(), l1.data(), C, fv.data());
                for (uint64_t c = 0; c < C; c++)
                    cfg->counts[counts_off + c] = (uint64_t)fv[c * 8] | ((uint64_t)fv[c * 8 + 1] << 32);
            }
            counts_off += C;
        }
        uint64_t kept = 0;
        for (uint64_t c = 0; c < C; c++) kept += keep[c];
        if (cfg->level_children) cfg->level_children[lv] = C;
        if (cfg->level_kept) cfg->level_kept[lv] = kept;
        if (last) {
            rc = fhh_tree_prune_last(c0, keep.data(), C);
            if (rc) return rc;
            rc = fhh_tree_prune_last(c1, keep.data(), C);
            if (rc) return rc;
        } else {
            rc = prune_impl(c0, keep.data(), C);
            if (rc) return rc;
            rc = prune_impl(c1, keep.data(), C);
            if (rc) return rc;
        }
    }
    return FHH_OK;
}

}  // extern "C"
