// HIP kernels for gfx950 (MI355X): the per-level ibDCF key evaluation of
// sks-codes/fuzzyheavyhitters and the kernels around it.
//
//   k_expand        ibDCFKey::eval_bit for every (dim-prefix, client, side, dir)
//                   (ibDCF.rs:208-227, prg.rs:92-122, collect.rs:379-391). Integer/LDS bound.
//   k_eq_count      plaintext stand-in for the GC equality test: clients whose two share
//                   strings agree, per child (collect.rs:393-482 replaced)
//   k_share_planes  share-bit planes for the GC (collect.rs:393-418)
//   k_child_sums_fe* per-child sums of the share values: the in-process harness's simulated OT
//                   shares, or (ot_val set) the real protocol's garbled-table / C-OT outputs
//                   (collect.rs:439-501, 846-905; named k_sim_ot_fe before r06)
//   k_sum_fe*       per-child sums of host-provided FE / FE255 values (collect.rs:487-501)
//   k_keygen        batched gen_interval keygen (ibDCF.rs:84-173)
//   k_init_table    eval_init for every key (ibDCF.rs:229-236, collect.rs:67-92)
//   k_eval_paths    eval_ibDCF at given prefixes (ibDCF.rs:238-250): fhh_tree_init_at's frontier
//   k_keys_from_aos add_key wire layout -> SoA device layout
#include "fhh_internal.h"
#include "expand_kernel.h"
#include "bincode_span.h"
#include "ball_src.h"
#include "../../include/fhh.h"
// The measured-negative k_expand forms of r01-r03 (bitsliced VALU AES, the T-table + pair-sliced
// hybrid, the earlier T-table variants) and their generated AES programs were removed in r06; they are
// in git history at commit 78c7ebe (fhh_expand_bs.hip, expand_ps.h, aes_bs_gen.h, aes_ps_gen.h,
// tools/gen_aes_bs.py, tools/gen_aes_ps.py). The build holds the product
// variant 52 and the generic-AES variant 33 the parity suite compares it with; the kernel switches
// only the removed forms used (draw-ahead, prefetch, wave timeline, end-of-launch phase, store
// diagnostics) are in history at commit 531b030.

namespace fhh {

__constant__ WordTable c_T0 = T0;

__device__ __forceinline__ uint32_t wave_id_uniform() {
    return __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
}

__device__ __forceinline__ void fill_table(uint32_t* tbl) {
    for (int i = threadIdx.x; i < kTableWords; i += blockDim.x) tbl[i] = c_T0.v[i / kTableReplicas];
    __syncthreads();
}

// --------------------------------------------------------------------------------------
// k_expand: one wave = 64 consecutive clients (one word) of one dim-j prefix group. Per entry
// and lane: 2 sides x 2 directions = 4 AES blocks in lockstep. CorWords of (level, dim, side,
// client) are loaded once per word of a work item and reused for the item's entries. Work items
// (item_layout) are drawn from atomic heads.
// --------------------------------------------------------------------------------------
typedef uint32_t v4u32_t __attribute__((ext_vector_type(4)));
using ExpandTab = Tab4T32<DevOpsX>;
constexpr int kExpandBlock = 1024;   // threads per workgroup: 16 waves share the 128 KiB of tables

// The entry loop's load and store order (A/B knobs, honoured like the others only in an explicit A/B build;
// DESIGN.md §5, profiles/gt_msg_batch/):
//   FHH_EXPAND_SLOAD     the wave-uniform words (live[], the parent t / y words, the item's cw_bits) are read
//                        through the scalar path, live[] one entry ahead: nothing in this launch writes them
//                        (an earlier launch's k_prune / k_expand did)
//   FHH_EXPAND_PREFETCH  entry e + 1's parent seeds and t / y words are requested after entry e's AES and before
//                        its stores (nothing is held across the AES): the wait at the loop's top then leaves the
//                        stores outstanding; as vmcnt counts loads and stores in one in-order counter, a load
//                        issued after them waits for their retirement too
// (One store from 8 lanes for the entry's 8 child t / y words, instead of 8 lane-0 stores, measured +2.8 % on its
// own and nothing on top of the two above: not kept, profiles/AB_HISTORY.md.)
#ifndef FHH_EXPAND_SLOAD
#define FHH_EXPAND_SLOAD 1
#endif
#ifndef FHH_EXPAND_PREFETCH
#define FHH_EXPAND_PREFETCH 1
#endif

// p[i] for a wave-uniform i, of words no kernel of this launch writes: a scalar load (constant address space)
template <typename T>
__device__ __forceinline__ T uniform_load(const T* p, size_t i) {
#if FHH_EXPAND_SLOAD
    return ((const __attribute__((address_space(4))) T*)p)[i];
#else
    return p[i];
#endif
}

// Word w (clients 64 w .. 64 w + 63) of entries [e_begin, e_end) of job J.
// Child seeds are written with the nontemporal hint: they are read again only at the next level,
// and 1.3 GB per launch left dirty in L2 costs a writeback at every kernel boundary.
// PAIR: sibling-pair AES (dir 0 / dir 1 share rounds 1-2, aes0_mmo_pair) instead of the generic one.
// NTL: parent seeds read with the nontemporal hint (each is read once per level; the CWs are
// re-read by every entry group of the level and should keep the L2).
template <bool PAIR, bool NTL>
__device__ __forceinline__ void expand_word(const ExpandJob& J, uint32_t w, uint32_t e_begin, uint32_t e_end,
                                            const uint32_t* tbl, uint32_t lane, uint32_t b0, uint32_t b1) {
    constexpr bool kPrefetch = FHH_EXPAND_PREFETCH, kAhead = FHH_EXPAND_SLOAD || FHH_EXPAND_PREFETCH;
    const uint32_t c = w * 64 + lane;
    const size_t npad = J.npad, nw = J.nw;
    if (e_begin >= e_end) return;

    // CorWord for (level, dim, side) — ibDCF.rs:215-217 `cor_words[state.level]`
    const size_t krow = (size_t)J.level * J.K + 2 * J.dim;
    uint4 cw[2];
    uint64_t cwp[2][4];
#pragma unroll
    for (int s = 0; s < 2; s++) {
        cw[s] = J.cw_seed[(krow + s) * npad + c];
#pragma unroll
        for (int b = 0; b < 4; b++) cwp[s][b] = uniform_load(J.cw_bits, ((krow + s) * 4 + b) * nw + w);
    }

    uint4 sd[2];   // the entry's parent seeds and t / y words
    uint64_t tw[2], yw[2];
    auto fetch = [&](uint32_t src) __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < 2; s++) {
            if constexpr (NTL) {
                const v4u32_t v = __builtin_nontemporal_load(
                    reinterpret_cast<const v4u32_t*>(J.src_seed + ((size_t)src * 2 + s) * npad + c));
                sd[s] = make_uint4(v[0], v[1], v[2], v[3]);
            } else {
                sd[s] = J.src_seed[((size_t)src * 2 + s) * npad + c];
            }
            tw[s] = uniform_load(J.src_t, ((size_t)src * 2 + s) * nw + w);
            yw[s] = uniform_load(J.src_y, ((size_t)src * 2 + s) * nw + w);
        }
    };
    // (nothing reads live[] at or beyond e_end <= n_live)
    uint32_t src = kAhead ? uniform_load(J.live, e_begin) : 0u;
    if constexpr (kPrefetch) {
        fetch(src);
        // (the CorWord loads are waited for here, once per word: still pending at the loop's head, they cost every
        // entry a wait for all loads at their use behind the AES, the next entry's request included)
        asm volatile("" ::"v"(cw[0].x), "v"(cw[1].x));
    }

    for (uint32_t e = e_begin; e < e_end; e++) {
        if constexpr (!kAhead) src = J.live[e];
        if constexpr (!kPrefetch) fetch(src);
        const bool more = e + 1 < e_end;   // wave-uniform
        if (kAhead && more) src = uniform_load(J.live, e + 1);
        uint32_t blk[4][4];     // index s * 2 + dir
        uint64_t pb[4], py[4];  // PRG control bits (tau.bits / tau.y_bits) as ballot planes
#pragma unroll
        for (int s = 0; s < 2; s++) {
            const uint32_t sw[4] = {sd[s].x, sd[s].y, sd[s].z, sd[s].w};
#pragma unroll
            for (int dir = 0; dir < 2; dir++) {
                prg_ctr(sw, dir, blk[s * 2 + dir]);
                uint32_t bit, ybit;
                prg_ctrl_bits(blk[s * 2 + dir][0], dir, bit, ybit);
                pb[s * 2 + dir] = __ballot(bit);
                py[s * 2 + dir] = __ballot(ybit);
            }
        }

        if constexpr (PAIR) aes0_mmo_pair<DevOpsX, ExpandTab, 4>(blk, tbl, b0, b1);
        else aes0_mmo_tab<DevOpsX, ExpandTab, 4>(blk, tbl, b0, b1);

        // child row de = (2 e + dir) 2 + s = 4 e + q, q = 2 dir + s
        v4u32_t out[4];
        uint64_t tq[4], yq[4];
#pragma unroll
        for (int s = 0; s < 2; s++) {
            const uint32_t tmask = 0u - (uint32_t)((tw[s] >> lane) & 1);   // if state.bit
#pragma unroll
            for (int dir = 0; dir < 2; dir++) {
                const uint32_t* o = blk[s * 2 + dir];
                out[2 * dir + s] = v4u32_t{o[0] ^ (cw[s].x & tmask), o[1] ^ (cw[s].y & tmask), o[2] ^ (cw[s].z & tmask),
                                           o[3] ^ (cw[s].w & tmask)};
                // new_bit = tau.bits[dir] ^ (t & cw.bits[dir]);
                // new_y = tau.y_bits[dir] ^ (t & cw.y_bits[dir]) ^ y   (ibDCF.rs:211-219)
                tq[2 * dir + s] = pb[s * 2 + dir] ^ (tw[s] & cwp[s][dir]);
                yq[2 * dir + s] = py[s * 2 + dir] ^ (tw[s] & cwp[s][2 + dir]) ^ yw[s];
            }
        }
        // The child t / y words go first, then the next entry's parent words are requested, then the 4 child
        // seeds are stored: behind the request stand exactly 4 stores on every path, so the counted wait at the
        // loop's top leaves all of them outstanding (a store in a lane-masked region behind the request is
        // counted along the path that skips it, and the wait then takes the first stores with it).
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                J.dst_t[((size_t)4 * e + q) * nw + w] = tq[q];
                J.dst_y[((size_t)4 * e + q) * nw + w] = yq[q];
            }
        }
        if (kPrefetch && more) fetch(src);
#pragma unroll
        for (int q = 0; q < 4; q++)
            __builtin_nontemporal_store(out[q], reinterpret_cast<v4u32_t*>(J.dst_seed + ((size_t)4 * e + q) * npad + c));
    }
}

// The two built forms differ in three switches (any other combination is simply not instantiated):
// PAIR / NTL: expand_word's AES form and parent-seed loads.
// MW: an item may span wpi consecutive words (item_layout, narrow levels), and each wave's first
// item is its wave index instead of a counter draw (the counter then hands out items from nwaves
// on: 4 096 simultaneous first draws cost ≈ 46 µs at the counter's 88 per µs). Without MW every
// item is one word and every item is drawn.
template <bool PAIR, bool MW, bool NTL>
__global__ __launch_bounds__(kExpandBlock, 1) void k_expand(ExpandLaunch a, uint32_t* work_counter) {
    __shared__ uint32_t tbl[ExpandTab::kWords];
    __shared__ uint32_t s_drained;   // bit h: a wave of this workgroup found head h dry
    for (int i = threadIdx.x; i < ExpandTab::kWords; i += kExpandBlock) tbl[i] = ExpandTab::word(c_T0.v, i);
    if (threadIdx.x == 0) s_drained = 0;
    __syncthreads();

    const uint32_t lane = threadIdx.x & 63;
    uint32_t b0, b1;
    ExpandTab::bases(lane, b0, b1);
    const uint64_t wpb = kExpandBlock / 64;
    const uint64_t nwaves = (uint64_t)gridDim.x * wpb;
    // sizes: kernel arguments (host-driven crawl) or LoopCtl (device-resident loop)
    const LoopCtl* ctl = a.ctl;
    const uint64_t total = ctl ? (ctl->abort ? 0 : ctl->total_items) : a.total_items;
    const uint32_t wpi = MW ? __builtin_amdgcn_readfirstlane(ctl ? ctl->wpi : a.wpi) : 1u;
    // Dynamic items come from H heads, one per XCD (blocks b and b + 8 share an XCD: one word
    // saturates at ≈88 dequeues/µs, 8 per-XCD heads do not), head h handing out items
    // draw_base + h + H·v. A block draws from its own head first, then from the others once they
    // run dry. The heads of a launch alternate between two sets by launch number: the first block
    // zeroes the other set for the next launch on the stream (the previous launch, done, used it),
    // so there is no exit count (4 096 same-address exit atomics alone cost ≈46 µs per launch).
    constexpr uint32_t H = kExpandHeads;
    uint32_t* heads = work_counter + kExpandSlot0 + (a.seq & 1) * H * kExpandSlotStride;
    if (blockIdx.x == 0 && threadIdx.x < H)
        atomicExch(work_counter + kExpandSlot0 + ((a.seq + 1) & 1) * H * kExpandSlotStride +
                       threadIdx.x * kExpandSlotStride, 0u);
    // (MW: wide levels, one-word items, keep one head — the per-XCD split measured ≈1 % slower there)
    const uint32_t nh = MW ? (wpi > 1 ? H : 1u) : H;
    const uint32_t home = blockIdx.x & (nh - 1);
    const uint64_t draw_base = MW ? nwaves : 0;   // the first nwaves items are dealt statically (MW)
    // lane 0 draws; bit h of s_drained: a wave of this block found head h dry (its siblings skip it)
    auto draw = [&]() -> uint64_t {
        uint64_t it = total;
        if (lane == 0) {
            for (uint32_t k = 0; k < nh; k++) {
                const uint32_t h = (home + k) & (nh - 1);
                if ((*(volatile uint32_t*)&s_drained >> h) & 1u) continue;
                const uint32_t v = atomicAdd(heads + h * kExpandSlotStride, 1u);
                const uint64_t cand = draw_base + h + (uint64_t)nh * v;
                if (cand < total) {
                    it = cand;
                    break;
                }
                atomicOr(&s_drained, 1u << h);
            }
        }
        return ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(it >> 32)) << 32) |
               __builtin_amdgcn_readfirstlane((uint32_t)it);
    };
    uint64_t item = MW ? (uint64_t)blockIdx.x * wpb + wave_id_uniform() : draw();
    while (item < total) {
        uint32_t ji = 0;
        if (ctl) {
            while (ji + 1 < a.njobs && item >= ctl->item_begin[ji + 1]) ji++;
        } else {
            while (ji + 1 < a.njobs && item >= a.job[ji + 1].item_begin) ji++;
        }
        ExpandJob J = a.job[ji];
        if (ctl) {
            J.n_live = ctl->n_live[ji % a.jobs_per_ctx];
            J.group = ctl->group;
            J.item_begin = ctl->item_begin[ji];
        }
        const ItemRange r = item_range(item - J.item_begin, J.n_live, J.nw, J.group, wpi);
        for (uint32_t w = r.w0; w < r.w1; w++) expand_word<PAIR, NTL>(J, w, r.e0, r.e1, tbl, lane, b0, b1);
        item = draw();
    }
}

// Variant table (fhh_set_variant): id, PAIR, MW, NTL, then item_layout's caps for the form — entries
// per item (the CorWord reuse against the wait for the launch's slowest wave) and words per item
// (above 1 only with MW). 52 is the product default, 33 the generic-AES form the parity suite
// compares it with; every other id is refused.
#define FHH_EXPAND_VARIANTS(X)      \
    X(33, false, false, false, 16, 1) \
    X(52, true, true, true, 16, 16)

struct VariantInfo {
    const void* fn;
    int threads;
    uint32_t max_group, max_wpi;
    const char* name;
};

static VariantInfo variant_info(int v) {
    switch (v) {
#define FHH_CASE(id, PAIR, MW, NTL, MAXG, MAXW) \
    case id: return VariantInfo{reinterpret_cast<const void*>(&k_expand<PAIR, MW, NTL>), kExpandBlock, MAXG, MAXW, ExpandTab::kName};
        FHH_EXPAND_VARIANTS(FHH_CASE)
#undef FHH_CASE
        default: return VariantInfo{nullptr, 0, 0, 0, ""};
    }
}

int expand_variant_count() { return 53; }   // ids 0..52; this build holds 33 and 52

const char* expand_variant_name(int v) { return variant_info(v).name; }

hipError_t launch_expand(const ExpandLaunch& a0, int variant, int grid, uint32_t* work_counter, uint32_t* seq,
                         hipStream_t stream) {
    if (a0.total_items == 0) return hipSuccess;
    ExpandLaunch a = a0;
    // the head set of this launch is chosen by the sequence's parity, and the launch zeroes the other
    // set for the next one (fhh_create zeroes both): the sequence advances only once a launch has been
    // enqueued, so a refused or failed launch cannot make the next one draw from a set the launch before
    // used up
    a.seq = *seq;
    const uint64_t wpb = kExpandBlock / 64;
    const uint64_t blocks_needed = (a.total_items + wpb - 1) / wpb;
    // device-resident loop: the item count is only known on the device -> full persistent grid
    const int g = a.ctl ? grid : (int)(blocks_needed < (uint64_t)grid ? blocks_needed : (uint64_t)grid);
    switch (variant) {
#define FHH_CASE(id, PAIR, MW, NTL, MAXG, MAXW) \
    case id: hipLaunchKernelGGL((k_expand<PAIR, MW, NTL>), dim3(g), dim3(kExpandBlock), 0, stream, a, work_counter); break;
        FHH_EXPAND_VARIANTS(FHH_CASE)
#undef FHH_CASE
        default: return hipErrorInvalidValue;
    }
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) ++*seq;
    return e;
}

int expand_grid(int device, int variant) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) cus = 256;
    const VariantInfo vi = variant_info(variant);
    int per_cu = 0;
    const size_t dyn = 0;
    if (!vi.fn || hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, vi.fn, vi.threads, dyn) != hipSuccess ||
        per_cu <= 0)
        per_cu = 1;
    return cus * per_cu;
}

int expand_threads(int variant) { return variant_info(variant).threads; }
uint32_t expand_max_group(int variant) { return variant_info(variant).max_group; }
uint32_t expand_max_wpi(int variant) { return variant_info(variant).max_wpi; }

// --------------------------------------------------------------------------------------
// Child-level kernels (one block per child, grid-stride).
// --------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <int NV>
__device__ __forceinline__ void block_sum_u64(uint64_t (&v)[NV], uint64_t* red /*[NV][kReduceThreads/64]*/) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nwv = blockDim.x >> 6;
#pragma unroll
    for (int k = 0; k < NV; k++) v[k] = wave_sum_u64(v[k]);
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < NV; k++) red[k * (kReduceThreads / 64) + wid] = v[k];
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < NV; k++) {
            uint64_t s = 0;
            for (int i = 0; i < nwv; i++) s += red[k * (kReduceThreads / 64) + i];
            v[k] = s;
        }
    }
    __syncthreads();
}

__device__ __forceinline__ uint64_t child_count(const ChildArgs& a) {
    return a.ctl ? (a.ctl->abort ? 0 : a.ctl->C) : a.C;
}

// the children a windowed kernel (GC + OT glue) visits: [c_off, min(C, c_off + c_cnt))
__device__ __forceinline__ uint64_t child_end(const ChildArgs& a) {
    const uint64_t C = child_count(a);
    if (!a.c_cnt) return C;
    const uint64_t e = a.c_off + a.c_cnt;
    return e < C ? e : C;
}

__device__ __forceinline__ void child_entries(const ChildArgs& a, uint64_t c, uint32_t (&e)[kMaxDims]) {
    const uint64_t p = c >> a.d;
    const uint32_t i = (uint32_t)(c & ((1u << a.d) - 1));
#pragma unroll
    for (int j = 0; j < kMaxDims; j++)
        if (j < (int)a.d) e[j] = 2 * a.parent_pos[p * a.d + j] + ((i >> j) & 1);
}

// eq word: bit = 1 iff the client's share string is identical on both servers
__device__ __forceinline__ uint64_t eq_word(const ChildArgs& a, const uint32_t (&e)[kMaxDims], uint32_t w) {
    uint64_t m = a.valid[w];
#pragma unroll
    for (int j = 0; j < kMaxDims; j++) {
        if (j < (int)a.d) {
#pragma unroll
            for (int s = 0; s < 2; s++) {
                const size_t idx = ((size_t)e[j] * 2 + s) * a.nw + w;
                const uint64_t e0 = a.s0.t[j][idx] ^ a.s0.y[j][idx];
                const uint64_t e1 = a.s1.t[j][idx] ^ a.s1.y[j][idx];
                m &= ~(e0 ^ e1);
            }
        }
    }
    return m;
}

// 1024 threads per child and two words per thread per pass, both words' loads issued before
// either popcount: at configs[1] (nw = 1563) one pass covers a child, so the kernel is one
// round of load latency instead of six dependent ones (r01: 10 us per level at 256 threads)
constexpr int kEqThreads = 1024;
__global__ __launch_bounds__(kEqThreads) void k_eq_count(ChildArgs a, uint64_t* counts) {
    __shared__ uint64_t red[kEqThreads / 64];
    const uint64_t C_ = child_count(a);
    for (uint64_t c = blockIdx.x; c < C_; c += gridDim.x) {
        uint32_t e[kMaxDims];
        child_entries(a, c, e);
        uint64_t v[1] = {0};
        for (uint32_t w = threadIdx.x; w < a.nw; w += 2 * kEqThreads) {
            const uint32_t w1 = w + kEqThreads;
            const uint64_t m0 = eq_word(a, e, w);
            const uint64_t m1 = w1 < a.nw ? eq_word(a, e, w1) : 0;
            v[0] += __popcll(m0) + __popcll(m1);
        }
        block_sum_u64<1>(v, red);
        if (threadIdx.x == 0) counts[c] = v[0];
    }
}

static int child_grid(uint64_t C) { return (int)(C < 65535 ? (C ? C : 1) : 65535); }
static uint64_t window_cap(const ChildArgs& a) { return a.c_cnt && a.c_cnt < a.C ? a.c_cnt : a.C; }

hipError_t launch_eq_count(const ChildArgs& a, uint64_t* counts, hipStream_t stream) {
    if (a.C == 0) return hipSuccess;
    hipLaunchKernelGGL(k_eq_count, dim3(child_grid(a.C)), dim3(kEqThreads), 0, stream, a, counts);
    return hipGetLastError();
}

// out [C][2d][nw]: left dims then right dims, E = y ^ t (collect.rs:399-405); with a child window
// (c_cnt > 0) only children [c_off, c_off + c_cnt), at rows c - c_off
__global__ __launch_bounds__(kReduceThreads) void k_share_planes(ChildArgs a, uint64_t* out) {
    const uint64_t C_ = child_end(a);
    for (uint64_t c = a.c_off + blockIdx.x; c < C_; c += gridDim.x) {
        uint32_t e[kMaxDims];
        child_entries(a, c, e);
        const uint32_t pnw = a.plane_nw ? a.plane_nw : a.nw;
        for (uint32_t w = threadIdx.x; w < pnw; w += blockDim.x) {
#pragma unroll
            for (int s = 0; s < 2; s++)
#pragma unroll
                for (int j = 0; j < kMaxDims; j++)
                    if (j < (int)a.d) {
                        const size_t idx = ((size_t)e[j] * 2 + s) * a.nw + w;
                        out[((size_t)(c - a.c_off) * 2 * a.d + (size_t)s * a.d + j) * pnw + w] =
                            w < a.nw ? (a.s0.t[j][idx] ^ a.s0.y[j][idx]) & a.valid[w] : 0ull;
                    }
        }
    }
}

hipError_t launch_share_planes(const ChildArgs& a, uint64_t* out, hipStream_t stream) {
    if (a.C == 0) return hipSuccess;
    hipLaunchKernelGGL(k_share_planes, dim3(child_grid(window_cap(a))), dim3(kReduceThreads), 0, stream, a, out);
    return hipGetLastError();
}

// ---- simulated OT share values --------------------------------------------------------
// PRF: mix64 chain (SplitMix64 finaliser) over (seed, level, child, client, word).
__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

constexpr uint64_t kFeP = (1ull << 62) - (1ull << 30) - 1;

// the equality bit the OT conversion consumes: plaintext (t, y) comparison, or in GC mode the
// evaluator's garbled-circuit output XOR the garbler's mask (the OT receiver's choice bit and
// the sender's message order, collect.rs:437-471: the received value is r0 iff eq)
__device__ __forceinline__ bool sim_eq_bit(const ChildArgs& a, const uint32_t (&e)[kMaxDims], uint64_t c, uint32_t i) {
    if (a.gc_out) return ((a.gc_out[(c - a.c_off) * a.gc_N + i] ^ a.gc_mask) & 1u) != 0;
    return (eq_word(a, e, i >> 6) >> (i & 63)) & 1;
}

// grid (children, client chunks of kSimOtChunk): one child per block row would leave the chip
// at ~3 waves per CU for the usual few hundred children (255 µs per level at configs[1]); the
// chunks' limb sums meet in partials by 64-bit atomics (zeroed by the launcher)
constexpr uint32_t kSimOtChunk = 16 * kReduceThreads;
__global__ __launch_bounds__(kReduceThreads) void k_child_sums_fe(ChildArgs a, uint64_t* partials) {
    __shared__ uint64_t red[4 * (kReduceThreads / 64)];
    const uint64_t base = mix64(a.prf_seed ^ a.level);
    const uint64_t C_ = child_end(a);
    const uint32_t i_begin = blockIdx.y * kSimOtChunk;
    const uint32_t i_end = min(i_begin + kSimOtChunk, a.n);
    for (uint64_t c = a.c_off + blockIdx.x; c < C_; c += gridDim.x) {
        uint32_t e[kMaxDims];
        child_entries(a, c, e);
        const uint64_t bc = mix64(base ^ c);
        uint64_t v[4] = {0, 0, 0, 0};
        for (uint32_t i = i_begin + threadIdx.x; i < i_end; i += blockDim.x) {
            uint64_t r1, v1;
            if (a.ot_val[0]) {   // the correlated OT's node values (OtArgs mode 2): garbler v + mask, receiver
                const size_t t = (c - a.c_off) * a.gc_N + i;
                r1 = static_cast<const uint64_t*>(a.ot_val[0])[t];
                v1 = static_cast<const uint64_t*>(a.ot_val[1])[t];
            } else {             // simulated OT shares (ideal OT harness)
                uint64_t r0 = mix64(mix64(bc ^ (a.client_base + i)) ^ 0ull) & ((1ull << 62) - 1);
                if (r0 >= kFeP) r0 -= kFeP;
                r1 = (r0 + 1 == kFeP) ? 0 : r0 + 1;              // r1 = r0 + one (collect.rs:443-444)
                v1 = sim_eq_bit(a, e, c, i) ? r0 : r1;           // receiver gets pair[o] (A.5)
            }
            v[0] += r1 & 0xFFFFFFFFull;
            v[1] += r1 >> 32;
            v[2] += v1 & 0xFFFFFFFFull;
            v[3] += v1 >> 32;
        }
        block_sum_u64<4>(v, red);
        if (threadIdx.x == 0)
            for (int k = 0; k < 4; k++) atomicAdd(reinterpret_cast<unsigned long long*>(partials + c * 4 + k), v[k]);
    }
}

hipError_t launch_child_sums_fe(const ChildArgs& a, uint64_t* partials, hipStream_t stream, bool zero) {
    if (a.C == 0) return hipSuccess;
    if (zero) {
        const hipError_t e = hipMemsetAsync(partials, 0, (size_t)a.C * 4 * sizeof(uint64_t), stream);
        if (e != hipSuccess) return e;
    }
    const uint32_t chunks = a.n ? (a.n + kSimOtChunk - 1) / kSimOtChunk : 1;
    hipLaunchKernelGGL(k_child_sums_fe, dim3(child_grid(window_cap(a)), chunks), dim3(kReduceThreads), 0, stream, a,
                       partials);
    return hipGetLastError();
}

// 255-bit helpers on 4 x u64 little-endian
__device__ __forceinline__ void fe255_canon(uint64_t (&x)[4]) {
    // x < 2^255; subtract p = 2^255 - 19 when x >= p (i.e. x + 19 carries into bit 255)
    uint64_t t[4];
    unsigned __int128 acc = (unsigned __int128)x[0] + 19;
    t[0] = (uint64_t)acc;
    acc = (unsigned __int128)x[1] + (uint64_t)(acc >> 64);
    t[1] = (uint64_t)acc;
    acc = (unsigned __int128)x[2] + (uint64_t)(acc >> 64);
    t[2] = (uint64_t)acc;
    acc = (unsigned __int128)x[3] + (uint64_t)(acc >> 64);
    t[3] = (uint64_t)acc;
    if (t[3] >> 63) {
        x[0] = t[0];
        x[1] = t[1];
        x[2] = t[2];
        x[3] = t[3] & 0x7FFFFFFFFFFFFFFFull;
    }
}

// BlockPair <-> 4 x u64 little-endian limbs: the value's 32 big-endian bytes, block 0 = bytes
// 0..15 (limbs 3, 2), block 1 = bytes 16..31 (limbs 1, 0) (field.rs:465-492); a block's 16
// bytes as four little-endian u32 words
__device__ __forceinline__ uint4 limbs_to_block(uint64_t hi, uint64_t lo) {
    return make_uint4(__builtin_bswap32((uint32_t)(hi >> 32)), __builtin_bswap32((uint32_t)hi),
                      __builtin_bswap32((uint32_t)(lo >> 32)), __builtin_bswap32((uint32_t)lo));
}
__device__ __forceinline__ void blockpair_to_limbs(uint4 b0, uint4 b1, uint64_t (&r)[4]) {
    r[3] = ((uint64_t)__builtin_bswap32(b0.x) << 32) | __builtin_bswap32(b0.y);
    r[2] = ((uint64_t)__builtin_bswap32(b0.z) << 32) | __builtin_bswap32(b0.w);
    r[1] = ((uint64_t)__builtin_bswap32(b1.x) << 32) | __builtin_bswap32(b1.y);
    r[0] = ((uint64_t)__builtin_bswap32(b1.z) << 32) | __builtin_bswap32(b1.w);
}

__global__ __launch_bounds__(kReduceThreads) void k_child_sums_fe255(ChildArgs a, uint64_t* partials) {
    __shared__ uint64_t red[16 * (kReduceThreads / 64)];
    const uint64_t base = mix64(a.prf_seed ^ a.level);
    const uint64_t C_ = child_end(a);
    for (uint64_t c = a.c_off + blockIdx.x; c < C_; c += gridDim.x) {
        uint32_t e[kMaxDims];
        child_entries(a, c, e);
        const uint64_t bc = mix64(base ^ c);
        uint64_t v[16];
#pragma unroll
        for (int k = 0; k < 16; k++) v[k] = 0;
        for (uint32_t i = threadIdx.x; i < a.n; i += blockDim.x) {
            uint64_t r1[4], got[4];
            if (a.ot_val[0]) {   // the correlated OT's node values (OtArgs mode 3), BlockPairs; the receiver's
                                 // unreduced, as FieldElm::try_from(BlockPair) reads them (field.rs:466-476)
                const size_t t = (c - a.c_off) * a.gc_N + i;
                const uint4* g = static_cast<const uint4*>(a.ot_val[0]);
                const uint4* r = static_cast<const uint4*>(a.ot_val[1]);
                blockpair_to_limbs(g[2 * t], g[2 * t + 1], r1);
                blockpair_to_limbs(r[2 * t], r[2 * t + 1], got);
            } else {             // simulated OT shares (ideal OT harness)
                const bool eq = sim_eq_bit(a, e, c, i);
                const uint64_t bi = mix64(bc ^ (a.client_base + i));
                uint64_t r0[4];
#pragma unroll
                for (int k = 0; k < 4; k++) r0[k] = mix64(bi ^ (uint64_t)k);
                r0[3] &= 0x7FFFFFFFFFFFFFFFull;
                fe255_canon(r0);
                // r1 = r0 + 1 mod p
                unsigned __int128 acc = (unsigned __int128)r0[0] + 1;
                r1[0] = (uint64_t)acc;
#pragma unroll
                for (int k = 1; k < 4; k++) {
                    acc = (unsigned __int128)r0[k] + (uint64_t)(acc >> 64);
                    r1[k] = (uint64_t)acc;
                }
                fe255_canon(r1);
#pragma unroll
                for (int k = 0; k < 4; k++) got[k] = eq ? r0[k] : r1[k];
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint64_t x1 = got[k];
                v[2 * k] += r1[k] & 0xFFFFFFFFull;
                v[2 * k + 1] += r1[k] >> 32;
                v[8 + 2 * k] += x1 & 0xFFFFFFFFull;
                v[8 + 2 * k + 1] += x1 >> 32;
            }
        }
        block_sum_u64<16>(v, red);
        if (threadIdx.x == 0)
            for (int k = 0; k < 16; k++) partials[c * 16 + k] = v[k];
    }
}

hipError_t launch_child_sums_fe255(const ChildArgs& a, uint64_t* partials, hipStream_t stream) {
    if (a.C == 0) return hipSuccess;
    hipLaunchKernelGGL(k_child_sums_fe255, dim3(child_grid(window_cap(a))), dim3(kReduceThreads), 0, stream, a, partials);
    return hipGetLastError();
}

// ---- per-child sums of the OT outputs (collect.rs:487-501, 891-905) ----------------------------
// Values [C][ld] in one of the FHH_VALS_* formats (include/fhh.h): host-provided u64 / u32 limbs
// (staged by the engine) or OT outputs left on the device (16-B blocks: an FE little-endian in
// bytes 0..7, fastfield.rs:414-431; a FieldElm as a BlockPair of 32 big-endian bytes,
// field.rs:465-492). Sums are 32-bit-limb partials in u64 (2^32 clients of headroom), reduced once
// on the host: [C][2] for FE, [C][8] for FE255 (the exact unreduced BigUint add_lazy sum).
__global__ __launch_bounds__(kReduceThreads) void k_sum_fe(const uint64_t* vals, uint64_t C, uint64_t n, uint64_t ld,
                                                          uint32_t stride, uint64_t* partials) {
    __shared__ uint64_t red[2 * (kReduceThreads / 64)];
    for (uint64_t c = blockIdx.x; c < C; c += gridDim.x) {
        uint64_t v[2] = {0, 0};
        for (uint64_t i = threadIdx.x; i < n; i += blockDim.x) {
            const uint64_t x = vals[(c * ld + i) * stride];
            v[0] += x & 0xFFFFFFFFull;
            v[1] += x >> 32;
        }
        block_sum_u64<2>(v, red);
        if (threadIdx.x == 0) {
            partials[c * 2] = v[0];
            partials[c * 2 + 1] = v[1];
        }
    }
}

template <bool BLOCKPAIR>
__global__ __launch_bounds__(kReduceThreads) void k_sum_fe255(const uint32_t* vals, uint64_t C, uint64_t n,
                                                             uint64_t ld, uint64_t* partials) {
    __shared__ uint64_t red[8 * (kReduceThreads / 64)];
    for (uint64_t c = blockIdx.x; c < C; c += gridDim.x) {
        uint64_t v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (uint64_t i = threadIdx.x; i < n; i += blockDim.x) {
            const uint4* p = reinterpret_cast<const uint4*>(vals + (c * ld + i) * 8);
            const uint4 lo = p[0], hi = p[1];
            if (BLOCKPAIR) {
                uint64_t r[4];
                blockpair_to_limbs(lo, hi, r);
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    v[2 * k] += r[k] & 0xFFFFFFFFull;
                    v[2 * k + 1] += r[k] >> 32;
                }
            } else {
                v[0] += lo.x; v[1] += lo.y; v[2] += lo.z; v[3] += lo.w;
                v[4] += hi.x; v[5] += hi.y; v[6] += hi.z; v[7] += hi.w;
            }
        }
        block_sum_u64<8>(v, red);
        if (threadIdx.x == 0)
            for (int k = 0; k < 8; k++) partials[c * 8 + k] = v[k];
    }
}

hipError_t launch_sum_vals(const void* vals, uint32_t fmt, uint64_t C, uint64_t n, uint64_t ld, uint64_t* partials,
                           hipStream_t stream) {
    if (C == 0) return hipSuccess;
    switch (fmt) {
        case FHH_VALS_FE_U64:
        case FHH_VALS_FE_BLOCK:
            hipLaunchKernelGGL(k_sum_fe, dim3(child_grid(C)), dim3(kReduceThreads), 0, stream,
                               static_cast<const uint64_t*>(vals), C, n, ld, fmt == FHH_VALS_FE_BLOCK ? 2u : 1u,
                               partials);
            break;
        case FHH_VALS_FE255_LIMBS:
            hipLaunchKernelGGL(k_sum_fe255<false>, dim3(child_grid(C)), dim3(kReduceThreads), 0, stream,
                               static_cast<const uint32_t*>(vals), C, n, ld, partials);
            break;
        case FHH_VALS_FE255_BLOCKPAIR:
            hipLaunchKernelGGL(k_sum_fe255<true>, dim3(child_grid(C)), dim3(kReduceThreads), 0, stream,
                               static_cast<const uint32_t*>(vals), C, n, ld, partials);
            break;
        default:
            return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// --------------------------------------------------------------------------------------
// k_keygen: one wave = 64 clients of one key (dim j, side). Restates gen_cor_word
// (ibDCF.rs:84-119) level by level; 4 AES blocks per level per lane (both seeds, both
// directions). Writes server 0's and server 1's key arrays (shared cor_words).
// SRC = where the key's bits alpha come from (one body, as the FE / Z_2^32 table kernels share theirs):
//   kKeygenBytes     the bounds as given, a byte per bit (fhh_gen_keys_pair)
//   kKeygenBallBits  the client's packed L-bit point a: alpha = a -/+ ball (gen_l_inf_ball, ibDCF.rs:175-188)
//   kKeygenCoords    the client's i16 (lat, long): alpha = clamp(c -/+ ball) (gen_l_inf_ball_from_coords, :189-205)
// The point forms (ball_src.h) read the point once per item: its low word and the carry's run before the level
// loop (ball_bound), then one 32-bit window per 32 levels; a level's bit comes from registers. A right bound that
// carries out of bit L lowers *a.bad to its (client, dim) index c d + j; its key is made from the wrapped sum and
// the host drops the whole call. With root_seeds = NULL the lane draws the 64 seed bytes of its (client, dim) as
// one ChaCha20 block: the left and the right item of a (client, dim) each compute the block and keep their half
// (~1 000 VALU ops beside an item's 4 L AES blocks; sharing it would cost a second pass or a pairing of items).
// --------------------------------------------------------------------------------------
template <int SRC>
__global__ __launch_bounds__(kExpandThreads) void k_keygen(KeygenArgs a) {
    __shared__ uint32_t tbl[kTableWords];
    fill_table(tbl);
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t lanebase = lane * 4;
    const uint64_t wpb = blockDim.x >> 6;
    const uint64_t nwaves = (uint64_t)gridDim.x * wpb;
    const uint64_t items = (uint64_t)a.K * a.nw;
    for (uint64_t item = (uint64_t)blockIdx.x * wpb + wave_id_uniform(); item < items; item += nwaves) {
        const uint32_t kk = (uint32_t)(item / a.nw);
        const uint32_t w = (uint32_t)(item % a.nw);
        const uint32_t j = kk >> 1, side_idx = kk & 1;
        const uint32_t side = side_idx == 0 ? 1u : 0u;   // left key: side=true, right: false (ibDCF.rs:170-171)
        const uint64_t c = (uint64_t)w * 64 + lane;
        const bool valid = c < a.n;
        const uint8_t* alpha = nullptr;   // kKeygenBytes: the bound; kKeygenBallBits: the point's row
        BallBound bound{0u, 0xFFFFFFFFu, false};
        uint32_t nb = 0, cur = 0;
        if constexpr (SRC == kKeygenBytes) {
            alpha = (side_idx == 0 ? a.left_bits : a.right_bits) + (valid ? (c * a.d + j) * a.L : 0);
        } else if constexpr (SRC == kKeygenBallBits) {
            nb = (a.L + 7) >> 3;
            alpha = a.points + (valid ? (c * a.d + j) * nb : 0);
            if (valid) {
                bound = ball_bound(alpha, a.L, a.ball, side_idx == 1);
                if (bound.carry_out) atomicMin(a.bad, (unsigned long long)(c * a.d + j));
            }
        } else {
            // L = 16 < 32: every level reads bound.low (ball_bit)
            if (valid) bound.low = coords_bound(reinterpret_cast<const int16_t*>(a.points)[c * 2 + j], j, a.ball, side_idx == 1);
        }

        uint32_t seed[2][4];
        if (SRC != kKeygenBytes && !a.root_seeds && valid) {
            uint32_t key[8], blk[16];
#pragma unroll
            for (int k = 0; k < 8; k++) key[k] = a.seed[k];
            chacha20_block(key, (a.seed_first + c) * a.d + j, blk);
            // words 0-7 (left) or 8-15 (right), picked by a mask: a ?: on the indices becomes a load from a
            // stack copy of the block
            const uint32_t right = 0u - side_idx;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                seed[0][k] = blk[k] ^ ((blk[k] ^ blk[8 + k]) & right);
                seed[1][k] = blk[4 + k] ^ ((blk[4 + k] ^ blk[12 + k]) & right);
            }
        } else if (valid) {
            const uint4* rs = reinterpret_cast<const uint4*>(a.root_seeds + ((c * a.d + j) * 2 + side_idx) * 32);
            const uint4 r0 = rs[0], r1 = rs[1];
            seed[0][0] = r0.x; seed[0][1] = r0.y; seed[0][2] = r0.z; seed[0][3] = r0.w;
            seed[1][0] = r1.x; seed[1][1] = r1.y; seed[1][2] = r1.z; seed[1][3] = r1.w;
        } else {
#pragma unroll
            for (int b = 0; b < 2; b++)
#pragma unroll
                for (int k = 0; k < 4; k++) seed[b][k] = 0;
        }
#pragma unroll
        for (int b = 0; b < 2; b++)
            a.root[b][(size_t)kk * a.npad + c] = make_uint4(seed[b][0], seed[b][1], seed[b][2], seed[b][3]);
        if (lane == 0) {
            a.key_idx[0][(size_t)kk * a.nw + w] = 0;         // key_idx = false
            a.key_idx[1][(size_t)kk * a.nw + w] = ~0ull;     // key_idx = true (ibDCF.rs:153-161)
        }
        uint32_t t[2] = {0u, 1u};                           // root_bits = (false, true), ibDCF.rs:140

        for (uint32_t l = 0; l < a.L; l++) {
            uint32_t bit;
            if constexpr (SRC == kKeygenBytes) {
                bit = valid ? (alpha[l] ? 1u : 0u) : 0u;
            } else {
                if (SRC == kKeygenBallBits && valid && (l & 31) == 0 && l + 32 < a.L) cur = ball_str32(alpha, nb, l);
                bit = valid ? ball_bit(bound, a.L, l, cur) : 0u;
            }
            uint32_t blk[4][4];                             // index b*2 + dir
            uint32_t pbit[4], pyb[4];
#pragma unroll
            for (int b = 0; b < 2; b++)
#pragma unroll
                for (int dir = 0; dir < 2; dir++) {
                    prg_ctr(seed[b], dir, blk[b * 2 + dir]);
                    prg_ctrl_bits(blk[b * 2 + dir][0], dir, pbit[b * 2 + dir], pyb[b * 2 + dir]);
                }
            aes0_mmo<DevOps, 4>(blk, tbl, lanebase);

            const uint32_t keep = bit, lose = bit ^ 1u;
            uint32_t cws[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t l0 = lose ? blk[1][k] : blk[0][k];
                const uint32_t l1 = lose ? blk[3][k] : blk[2][k];
                cws[k] = l0 ^ l1;                                   // ibDCF.rs:91
            }
            // data.b.bits.k = pbit[b*2+k], data.b.y_bits.k = pyb[b*2+k]
            const uint32_t cb0 = pbit[0] ^ pbit[2] ^ bit ^ 1u;       // :93
            const uint32_t cb1 = pbit[1] ^ pbit[3] ^ bit;            // :94
            const uint32_t cy0 = pyb[0] ^ pyb[2] ^ (bit & (side ^ 1u) & 1u);   // :97 bit & !side
            const uint32_t cy1 = pyb[1] ^ pyb[3] ^ ((bit ^ 1u) & side);        // :98 !bit & side
            const uint32_t cwb_keep = keep ? cb1 : cb0;
#pragma unroll
            for (int b = 0; b < 2; b++) {                            // :103-116
                const uint32_t tm = 0u - t[b];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const uint32_t kept = keep ? blk[b * 2 + 1][k] : blk[b * 2][k];
                    seed[b][k] = kept ^ (cws[k] & tm);
                }
                const uint32_t nb = (keep ? pbit[b * 2 + 1] : pbit[b * 2]) ^ (t[b] & cwb_keep);
                t[b] = nb;
            }
            const size_t row = (size_t)l * a.K + kk;
            const uint4 cwv = make_uint4(cws[0], cws[1], cws[2], cws[3]);
            a.cw_seed[0][row * a.npad + c] = cwv;
            a.cw_seed[1][row * a.npad + c] = cwv;
            const uint64_t q0 = __ballot(cb0), q1 = __ballot(cb1), q2 = __ballot(cy0), q3 = __ballot(cy1);
            if (lane == 0) {
                const uint64_t q[4] = {q0, q1, q2, q3};
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    a.cw_bits[0][(row * 4 + b) * a.nw + w] = q[b];
                    a.cw_bits[1][(row * 4 + b) * a.nw + w] = q[b];
                }
            }
        }
    }
}

hipError_t launch_keygen(const KeygenArgs& a, int src, hipStream_t stream) {
    const uint64_t items = (uint64_t)a.K * a.nw;
    if (items == 0) return hipSuccess;
    const uint64_t wpb = kExpandThreads / 64;
    uint64_t blocks = (items + wpb - 1) / wpb;
    if (blocks > 4096) blocks = 4096;
    const dim3 grid((unsigned)blocks), block(kExpandThreads);
    switch (src) {
        case kKeygenBytes:
            hipLaunchKernelGGL(k_keygen<kKeygenBytes>, grid, block, 0, stream, a);
            break;
        case kKeygenBallBits:
            hipLaunchKernelGGL(k_keygen<kKeygenBallBits>, grid, block, 0, stream, a);
            break;
        case kKeygenCoords:
            hipLaunchKernelGGL(k_keygen<kKeygenCoords>, grid, block, 0, stream, a);
            break;
        default:
            return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// --------------------------------------------------------------------------------------
// eval_init for dim `dim` -> entry 0 of that dim's table: seed = root_seed, t = y = key_idx
// --------------------------------------------------------------------------------------
__global__ void k_init_table(const uint4* root, const uint64_t* key_idx, uint32_t dim, uint32_t npad, uint32_t nw,
                             uint4* seed, uint64_t* t, uint64_t* y) {
    const uint64_t total = (uint64_t)2 * npad;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t s = (uint32_t)(i / npad), c = (uint32_t)(i % npad);
        seed[(size_t)s * npad + c] = root[((size_t)2 * dim + s) * npad + c];
        if (c < nw) {
            const uint64_t k = key_idx[((size_t)2 * dim + s) * nw + c];
            t[(size_t)s * nw + c] = k;
            y[(size_t)s * nw + c] = k;
        }
    }
}

hipError_t launch_init_tables(const uint4* root, const uint64_t* key_idx, uint32_t dim, uint32_t K, uint32_t npad,
                              uint32_t nw, uint4* seed, uint64_t* t, uint64_t* y, hipStream_t stream) {
    (void)K;
    const uint64_t total = (uint64_t)2 * npad;
    unsigned blocks = (unsigned)((total + 255) / 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_init_table, dim3(blocks), dim3(256), 0, stream, root, key_idx, dim, npad, nw, seed, t, y);
    return hipGetLastError();
}

// --------------------------------------------------------------------------------------
// k_eval_paths: eval_ibDCF (ibDCF.rs:238-250) of every client's keys at given prefixes — fhh_tree_init_at.
// One wave = 64 consecutive clients (word w) of one (dim j, side s, group of kEvalPathsP distinct dim-j
// prefixes); one lane = one client. The lane walks the group's prefixes from the root down `depth` levels
// with their seeds in registers: one AES block per (prefix, key, level), the 4 prefixes' blocks in lockstep
// (k_expand spends four per entry and level, both directions of both sides, and stores every child seed).
// The level's CorWord seed is loaded once for the 4 prefixes (4 B per AES block); its bit words, the t / y
// words and the direction bits (packed per prefix, bit l % 32 of word l / 32) are wave-uniform and go
// through the scalar path. Level l + 1's CorWord is requested before level l's AES. Lanes past n do what
// they do in k_init_table / k_expand: the same arithmetic on the padding's (zero) keys. A partial last
// group repeats its last prefix in the idle slots and stores only the prefixes that exist.
// k_expand's launch shape: 1024 threads share the 128 KiB of tables, 4 waves per SIMD; every item costs
// the same, so the items are dealt grid-stride.
// --------------------------------------------------------------------------------------
// Two forms of one body (as k_keygen's): kEvalAll is k_eval_paths, every word of the layout into entries
// 0 .. n_prefixes - 1; kEvalJoin is k_join_paths (fhh_join_clients_bincode), the words [w_first, w_first + words)
// only, prefix e into the table entry rows[e] (the dim's live list), and in the word the joiners share with the
// clients already there (first_mask != ~0) only their lanes: the seed stores predicated, the t / y words merged
// as (old & ~mask) | (new & mask), bincode_span.h's rule for the keys.
// --------------------------------------------------------------------------------------
constexpr int kEvalAll = 0;
constexpr int kEvalJoin = 1;
template <int FORM>
__device__ __forceinline__ void eval_paths_body(const EvalPathsArgs& a, const JoinPathsExtra& x) {
    __shared__ uint32_t tbl[ExpandTab::kWords];
    for (int i = threadIdx.x; i < ExpandTab::kWords; i += kExpandBlock) tbl[i] = ExpandTab::word(c_T0.v, i);
    __syncthreads();

    constexpr int P = kEvalPathsP;
    const uint32_t lane = threadIdx.x & 63;
    uint32_t b0, b1;
    ExpandTab::bases(lane, b0, b1);
    const uint64_t wpb = kExpandBlock / 64;
    const uint64_t nwaves = (uint64_t)gridDim.x * wpb;
    const size_t npad = a.npad, nw = a.nw;
    for (uint64_t item = (uint64_t)blockIdx.x * wpb + wave_id_uniform(); item < a.total_items; item += nwaves) {
        uint32_t j = 0;
        while (j + 1 < a.d && item >= a.job[j + 1].item_begin) j++;
        const EvalPathsJob& J = a.job[j];
        // item = (group * 2 + side) * nw + word: a workgroup's waves read neighbouring words of one CorWord row
        const uint64_t local = item - J.item_begin;
        uint32_t w, gs;
        if constexpr (FORM == kEvalJoin) {
            w = x.w_first + (uint32_t)(local % x.words);
            gs = (uint32_t)(local / x.words);
        } else {
            w = (uint32_t)(local % nw);
            gs = (uint32_t)(local / nw);
        }
        const uint32_t s = gs & 1u, e0 = (gs >> 1) * P;
        const uint32_t c = w * 64 + lane;
        const size_t kk = 2 * j + s;

        // eval_init (ibDCF.rs:229-236): seed = root_seed, t = y = key_idx
        const uint4 root = a.root_seed[kk * npad + c];
        const uint64_t kidx = uniform_load(a.key_idx, kk * nw + w);
        uint32_t sd[P][4];
        uint64_t tw[P], yw[P];
        const uint32_t* dirs[P];
#pragma unroll
        for (int p = 0; p < P; p++) {
            sd[p][0] = root.x; sd[p][1] = root.y; sd[p][2] = root.z; sd[p][3] = root.w;
            tw[p] = yw[p] = kidx;
            const uint32_t e = e0 + p < J.n_prefixes ? e0 + p : J.n_prefixes - 1;
            dirs[p] = J.dirs + (size_t)e * a.dir_words;
        }

        uint4 cw = make_uint4(0, 0, 0, 0);
        uint64_t cwp[4] = {0, 0, 0, 0};
        if (a.depth) {
            cw = a.cw_seed[kk * npad + c];
#pragma unroll
            for (int b = 0; b < 4; b++) cwp[b] = uniform_load(a.cw_bits, (kk * 4 + b) * nw + w);
        }
        uint32_t dw[P] = {};
        for (uint32_t l = 0; l < a.depth; l++) {
            if ((l & 31u) == 0) {
#pragma unroll
                for (int p = 0; p < P; p++) dw[p] = uniform_load(dirs[p], l >> 5);
            }
            // the next level's CorWord (ibDCF.rs:215-217 `cor_words[state.level]`), off the dependent chain
            uint4 cwn = cw;
            uint64_t cwpn[4] = {cwp[0], cwp[1], cwp[2], cwp[3]};
            if (l + 1 < a.depth) {
                const size_t krow = (size_t)(l + 1) * a.K + kk;
                cwn = a.cw_seed[krow * npad + c];
#pragma unroll
                for (int b = 0; b < 4; b++) cwpn[b] = uniform_load(a.cw_bits, (krow * 4 + b) * nw + w);
            }
            uint32_t blk[P][4];
            uint64_t pb[P], py[P];
            uint32_t dir[P];
#pragma unroll
            for (int p = 0; p < P; p++) {
                dir[p] = (dw[p] >> (l & 31u)) & 1u;
                prg_ctr(sd[p], (int)dir[p], blk[p]);
                uint32_t bit, ybit;
                prg_ctrl_bits(blk[p][0], (int)dir[p], bit, ybit);
                pb[p] = __ballot(bit);
                py[p] = __ballot(ybit);
            }
            aes0_mmo_tab<DevOpsX, ExpandTab, P>(blk, tbl, b0, b1);
#pragma unroll
            for (int p = 0; p < P; p++) {
                const uint32_t tmask = 0u - (uint32_t)((tw[p] >> lane) & 1);   // if state.bit
                sd[p][0] = blk[p][0] ^ (cw.x & tmask);
                sd[p][1] = blk[p][1] ^ (cw.y & tmask);
                sd[p][2] = blk[p][2] ^ (cw.z & tmask);
                sd[p][3] = blk[p][3] ^ (cw.w & tmask);
                // new_bit = tau.bits[dir] ^ (t & cw.bits[dir]);
                // new_y = tau.y_bits[dir] ^ (t & cw.y_bits[dir]) ^ y   (ibDCF.rs:211-219)
                const uint64_t cb = dir[p] ? cwp[1] : cwp[0], cy = dir[p] ? cwp[3] : cwp[2];
                yw[p] = py[p] ^ (tw[p] & cy) ^ yw[p];
                tw[p] = pb[p] ^ (tw[p] & cb);
            }
            cw = cwn;
#pragma unroll
            for (int b = 0; b < 4; b++) cwp[b] = cwpn[b];
        }

#pragma unroll
        for (int p = 0; p < P; p++) {
            const uint32_t e = e0 + p;
            if (e < J.n_prefixes) {   // wave-uniform
                if constexpr (FORM == kEvalJoin) {
                    const size_t row = (size_t)2 * uniform_load(x.rows[j], e) + s;
                    const uint64_t own = w == x.w_first ? x.first_mask : ~0ull;   // the lanes this launch writes
                    if ((own >> lane) & 1) J.dst_seed[row * npad + c] = make_uint4(sd[p][0], sd[p][1], sd[p][2], sd[p][3]);
                    if (lane == 0) {
                        uint64_t t = tw[p], y = yw[p];
                        if (own != ~0ull) {
                            t = (J.dst_t[row * nw + w] & ~own) | (t & own);
                            y = (J.dst_y[row * nw + w] & ~own) | (y & own);
                        }
                        J.dst_t[row * nw + w] = t;
                        J.dst_y[row * nw + w] = y;
                    }
                } else {
                    const size_t row = (size_t)2 * e + s;
                    J.dst_seed[row * npad + c] = make_uint4(sd[p][0], sd[p][1], sd[p][2], sd[p][3]);
                    if (lane == 0) {
                        J.dst_t[row * nw + w] = tw[p];
                        J.dst_y[row * nw + w] = yw[p];
                    }
                }
            }
        }
    }
}

__global__ __launch_bounds__(kExpandBlock, 1) void k_eval_paths(EvalPathsArgs a) {
    eval_paths_body<kEvalAll>(a, JoinPathsExtra{});
}

__global__ __launch_bounds__(kExpandBlock, 1) void k_join_paths(EvalPathsArgs a, JoinPathsExtra x) {
    eval_paths_body<kEvalJoin>(a, x);
}

hipError_t launch_eval_paths(const EvalPathsArgs& a, int grid, hipStream_t stream) {
    if (a.total_items == 0) return hipSuccess;
    const uint64_t wpb = kExpandBlock / 64;
    const uint64_t blocks_needed = (a.total_items + wpb - 1) / wpb;
    const int g = (int)(blocks_needed < (uint64_t)grid ? blocks_needed : (uint64_t)grid);
    hipLaunchKernelGGL(k_eval_paths, dim3(g), dim3(kExpandBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_join_paths(const EvalPathsArgs& a, const JoinPathsExtra& x, int grid, hipStream_t stream) {
    if (a.total_items == 0) return hipSuccess;
    if (x.words == 0 || (uint64_t)x.w_first + x.words > a.nw) return hipErrorInvalidValue;
    const uint64_t wpb = kExpandBlock / 64;
    const uint64_t blocks_needed = (a.total_items + wpb - 1) / wpb;
    const int g = (int)(blocks_needed < (uint64_t)grid ? blocks_needed : (uint64_t)grid);
    hipLaunchKernelGGL(k_join_paths, dim3(g), dim3(kExpandBlock), 0, stream, a, x);
    return hipGetLastError();
}

// --------------------------------------------------------------------------------------
// add_key wire layout (AoS, client-major) -> SoA. One wave = 64 clients of one (level, key).
// --------------------------------------------------------------------------------------
// fhh_add_keys (collect.rs:62 add_key, host AoS -> device SoA): an item is 8 consecutive levels of
// one key for 64 clients, so a lane reads its client's 128 contiguous bytes of CorWord seeds (one
// cache line, 16-B aligned: the AoS stride is L x 16 B) and 8 bits bytes, and the wave writes 8
// coalesced 1 KiB rows (one level per item read a 16-B sliver of 64 lines and came back to the same
// lines for the next 7 levels); the item past the last level block holds the roots / key_idx
__global__ void k_keys_from_aos(const uint8_t* key_idx, const uint8_t* root_seed, const uint8_t* cw_seed,
                                const uint8_t* cw_bits, uint64_t n, uint32_t K, uint32_t L, uint32_t npad, uint32_t nw,
                                uint4* d_cw_seed, uint64_t* d_cw_bits, uint4* d_root, uint64_t* d_key_idx) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wpb = blockDim.x >> 6;
    const uint64_t nwaves = (uint64_t)gridDim.x * wpb;
    const uint32_t nlb = (L + 7) / 8;
    const uint64_t items = (uint64_t)(nlb + 1) * K * nw;
    for (uint64_t item = (uint64_t)blockIdx.x * wpb + wave_id_uniform(); item < items; item += nwaves) {
        const uint32_t w = (uint32_t)(item % nw);
        const uint32_t kk = (uint32_t)((item / nw) % K);
        const uint32_t lb = (uint32_t)(item / ((uint64_t)nw * K));
        const uint64_t c = (uint64_t)w * 64 + lane;
        const bool valid = c < n;
        if (lb < nlb) {
            const uint32_t l0 = lb * 8, nl = min(8u, L - l0);
            const uint4* p = reinterpret_cast<const uint4*>(cw_seed) + (c * K + kk) * L + l0;
            const uint8_t* pb = cw_bits + (c * K + kk) * L + l0;
            uint4 v[8];
            uint32_t nib[8];
#pragma unroll
            for (int k = 0; k < 8; k++) {
                v[k] = (valid && (uint32_t)k < nl) ? p[k] : make_uint4(0, 0, 0, 0);
                nib[k] = (valid && (uint32_t)k < nl) ? pb[k] : 0u;
            }
#pragma unroll
            for (int k = 0; k < 8; k++) {
                if ((uint32_t)k >= nl) break;   // wave-uniform
                const size_t row = (size_t)(l0 + k) * K + kk;
                d_cw_seed[row * npad + c] = v[k];
                uint64_t q[4];
#pragma unroll
                for (int b = 0; b < 4; b++) q[b] = __ballot((nib[k] >> b) & 1);
                if (lane == 0)
#pragma unroll
                    for (int b = 0; b < 4; b++) d_cw_bits[(row * 4 + b) * nw + w] = q[b];
            }
        } else {
            uint4 v = make_uint4(0, 0, 0, 0);
            uint32_t ki = 0;
            if (valid) {
                const uint8_t* p = root_seed + (c * K + kk) * 16;
                uint32_t x[4];
                for (int k = 0; k < 4; k++)
                    x[k] = (uint32_t)p[4 * k] | ((uint32_t)p[4 * k + 1] << 8) | ((uint32_t)p[4 * k + 2] << 16) |
                           ((uint32_t)p[4 * k + 3] << 24);
                v = make_uint4(x[0], x[1], x[2], x[3]);
                ki = key_idx[c * K + kk] ? 1u : 0u;
            }
            d_root[(size_t)kk * npad + c] = v;
            const uint64_t q = __ballot(ki);
            if (lane == 0) d_key_idx[(size_t)kk * nw + w] = q;
        }
    }
}

// AddKeysRequest.keys (rpc.rs:12-15) in bincode 1.x legacy encoding (as `bincode::serialize`,
// leader.rs:101): u64 n, then per client u64 d and d x (ibDCFKey left, ibDCFKey right); an
// ibDCFKey (ibDCF.rs:16-21) = key_idx bool (1 B), root_seed (16 B), u64 L, L x CorWord
// (ibDCF.rs:9-14: seed 16 B, bits.0, bits.1, y_bits.0, y_bits.1 as 1-byte bools). Records
// are fixed-size, so every (level, key, 64-client word) item is decoded in place into the
// SoA device layout; malformed bools / lengths set bits of *err (bool > 1: 1, L: 2, d: 4).
__device__ __forceinline__ uint64_t load_u64_le(const uint8_t* p) {
    uint64_t v = 0;
    for (int i = 0; i < 8; i++) v |= (uint64_t)p[i] << (8 * i);
    return v;
}

__device__ __forceinline__ uint4 load_seed(const uint8_t* p) {
    uint32_t x[4];
    for (int k = 0; k < 4; k++)
        x[k] = (uint32_t)p[4 * k] | ((uint32_t)p[4 * k + 1] << 8) | ((uint32_t)p[4 * k + 2] << 16) |
               ((uint32_t)p[4 * k + 3] << 24);
    return make_uint4(x[0], x[1], x[2], x[3]);
}

// (one lane per client: the CW levels [l_first, L) byte by byte, then level L = roots / key_idx;
// the CW levels go through k_bincode_cw_tiles below, so the launch starts at l_first = L)
__global__ void k_keys_from_bincode(const uint8_t* buf, uint64_t n, uint32_t d, uint32_t L, uint32_t npad,
                                    uint32_t nw, uint4* d_cw_seed, uint64_t* d_cw_bits, uint4* d_root,
                                    uint64_t* d_key_idx, uint32_t* err, uint32_t l_first) {
    const uint32_t K = 2 * d;
    const uint64_t KB = 25 + 20ull * L;      // one serialized ibDCFKey
    const uint64_t R = 8 + (uint64_t)K * KB;  // one client: u64 d + d (left, right) pairs
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wpb = blockDim.x >> 6;
    const uint64_t nwaves = (uint64_t)gridDim.x * wpb;
    const uint64_t items = (uint64_t)(L + 1) * K * nw;   // level L = roots / key_idx
    for (uint64_t item = (uint64_t)l_first * K * nw + (uint64_t)blockIdx.x * wpb + wave_id_uniform(); item < items;
         item += nwaves) {
        const uint32_t w = (uint32_t)(item % nw);
        const uint32_t kk = (uint32_t)((item / nw) % K);
        const uint32_t l = (uint32_t)(item / ((uint64_t)nw * K));
        const uint64_t c = (uint64_t)w * 64 + lane;
        const bool valid = c < n;
        const uint8_t* rec = buf + 8 + c * R;
        const uint8_t* key = rec + 8 + (uint64_t)kk * KB;
        uint32_t bad = 0;
        if (l < L) {
            uint4 v = make_uint4(0, 0, 0, 0);
            uint32_t nib = 0;
            if (valid) {
                const uint8_t* cw = key + 25 + 20ull * l;
                v = load_seed(cw);
                for (int b = 0; b < 4; b++) {
                    const uint32_t x = cw[16 + b];
                    bad |= x > 1 ? 1u : 0u;
                    nib |= (x & 1u) << b;
                }
            }
            const size_t row = (size_t)l * K + kk;
            d_cw_seed[row * npad + c] = v;
            uint64_t q[4];
            for (int b = 0; b < 4; b++) q[b] = __ballot((nib >> b) & 1);
            if (lane == 0)
                for (int b = 0; b < 4; b++) d_cw_bits[(row * 4 + b) * nw + w] = q[b];
        } else {
            uint4 v = make_uint4(0, 0, 0, 0);
            uint32_t ki = 0;
            if (valid) {
                ki = key[0];
                bad |= ki > 1 ? 1u : 0u;
                v = load_seed(key + 1);
                bad |= load_u64_le(key + 17) != L ? 2u : 0u;
                if (kk == 0) bad |= load_u64_le(rec) != d ? 4u : 0u;
            }
            d_root[(size_t)kk * npad + c] = v;
            const uint64_t q = __ballot(ki & 1u);
            if (lane == 0) d_key_idx[(size_t)kk * nw + w] = q;
        }
        if (bad) atomicOr(err, bad);
    }
}

// The correction words as tiles of 64 clients x kBcLevels levels of one key: a client's window of
// the payload (20 B per level, at an arbitrary byte offset) is staged into LDS by contiguous aligned
// dword loads (644 B per client, one wave per client at a time), then each lane (= client) extracts
// its levels with v_alignbit and the tile leaves as 1 KiB rows of [level][key][client] seeds plus
// the bit-plane ballots. The byte-per-load form (one lane per client and level, 20 global_load_ubyte
// 20 KiB apart) reached 0.58 TB/s on 2 GB; row f4, rpc.rs:12-15.
constexpr int kBcLevels = 32;
constexpr int kBcRow = 5 * kBcLevels + 1;   // dwords staged per client (odd: conflict-free rows)
__global__ __launch_bounds__(256) void k_bincode_cw_tiles(const uint8_t* buf, uint64_t n, uint32_t d, uint32_t L,
                                                          uint32_t npad, uint32_t nw, uint4* d_cw_seed,
                                                          uint64_t* d_cw_bits, uint32_t* err) {
    __shared__ uint32_t st[64 * kBcRow];
    const uint32_t K = 2 * d;
    const uint64_t KB = 25 + 20ull * L, R = 8 + (uint64_t)K * KB;
    const uint32_t nlb = (L + kBcLevels - 1) / kBcLevels;
    const uint64_t tiles = (uint64_t)nw * K * nlb;
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint32_t w = (uint32_t)(tile % nw);
        const uint32_t kk = (uint32_t)((tile / nw) % K);
        const uint32_t l0 = (uint32_t)(tile / ((uint64_t)nw * K)) * kBcLevels;
        const uint32_t nl = min((uint32_t)kBcLevels, L - l0);
        // stage: wave wv takes clients wv + 4 i (i < 16); all 48 loads of a lane are issued before
        // the first LDS write (a load -> write pair per client serialised 16 HBM latencies per tile)
        uint32_t v[16][3];
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const uint64_t c = (uint64_t)w * 64 + wv + 4 * i;
            const uint64_t s0 = 8 + c * R + 8 + kk * KB + 25 + 20ull * l0;   // level l0's CorWord
            const uint64_t a0 = s0 & ~3ull;
            const uint32_t ndw = c < n ? (uint32_t)((s0 + 20ull * nl + 3 - a0) / 4) : 0u;   // <= kBcRow
            const uint32_t* src = reinterpret_cast<const uint32_t*>(buf + a0);
#pragma unroll
            for (int r = 0; r < 3; r++) {
                const uint32_t j = lane + 64 * r;
                v[i][r] = j < ndw ? src[j] : 0u;
            }
        }
#pragma unroll
        for (int i = 0; i < 16; i++)
#pragma unroll
            for (int r = 0; r < 3; r++) {
                const uint32_t j = lane + 64 * r;
                if (j < (uint32_t)kBcRow) st[(wv + 4 * i) * kBcRow + j] = v[i][r];
            }
        __syncthreads();
        const uint64_t c = (uint64_t)w * 64 + lane;
        const bool valid = c < n;
        const uint32_t sh = (uint32_t)((8 + c * R + 8 + kk * KB + 25 + 20ull * l0) & 3) * 8;
        uint32_t bad = 0;
        for (uint32_t li = wv; li < nl; li += 4) {
            uint4 v = make_uint4(0, 0, 0, 0);
            uint32_t nib = 0;
            if (valid) {
                const uint32_t* row = st + lane * kBcRow + 5 * li;   // 5 li + 5 < kBcRow
                uint32_t u[5];
#pragma unroll
                for (int k = 0; k < 5; k++) u[k] = __builtin_amdgcn_alignbit(row[k + 1], row[k], sh);
                v = make_uint4(u[0], u[1], u[2], u[3]);
#pragma unroll
                for (int b = 0; b < 4; b++) {   // bits.0, bits.1, y_bits.0, y_bits.1 as bincode bools
                    const uint32_t x = (u[4] >> (8 * b)) & 0xFFu;
                    bad |= x > 1 ? 1u : 0u;
                    nib |= (x & 1u) << b;
                }
            }
            const size_t rowi = (size_t)(l0 + li) * K + kk;
            d_cw_seed[rowi * npad + c] = v;
            uint64_t q[4];
#pragma unroll
            for (int b = 0; b < 4; b++) q[b] = __ballot((nib >> b) & 1);
            if (lane == 0)
#pragma unroll
                for (int b = 0; b < 4; b++) d_cw_bits[(rowi * 4 + b) * nw + w] = q[b];
        }
        if (bad) atomicOr(err, bad);
        __syncthreads();
    }
}

hipError_t launch_keys_from_bincode(const uint8_t* buf, uint64_t n, uint32_t d, uint32_t L, uint32_t npad, uint32_t nw,
                                    uint4* d_cw_seed, uint64_t* d_cw_bits, uint4* d_root, uint64_t* d_key_idx,
                                    uint32_t* err, hipStream_t stream) {
    int dev = 0, cus = 256;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    const uint64_t tiles = (uint64_t)nw * 2 * d * ((L + kBcLevels - 1) / kBcLevels);
    if (tiles) {
        const uint64_t cap = (uint64_t)cus * 8;
        hipLaunchKernelGGL(k_bincode_cw_tiles, dim3((unsigned)(tiles < cap ? tiles : cap)), dim3(256), 0, stream, buf,
                           n, d, L, npad, nw, d_cw_seed, d_cw_bits, err);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const uint64_t items = (uint64_t)2 * d * nw;   // level L: roots / key_idx / headers
    uint64_t blocks = (items + 3) / 4;
    if (blocks > 8192) blocks = 8192;
    if (blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(k_keys_from_bincode, dim3((unsigned)blocks), dim3(256), 0, stream, buf, n, d, L, npad, nw,
                       d_cw_seed, d_cw_bits, d_root, d_key_idx, err, L);
    return hipGetLastError();
}

// ---- appended add_keys batches (fhh_add_keys_bincode_append) -------------------------------------
// The two decode kernels above with a destination offset: record i of the batch (m records in buf, after its
// u64 count) lands on client c0 + i of a layout that already holds the clients below c0, so the word is
// floor((c0 + i) / 64), the lane (c0 + i) mod 64, and the batch's first and last words may be shared with
// other clients (bincode_span.h gives each word's lanes, source record and tail). Seed stores are predicated
// on the word's lanes + tail (the tail, the lanes after the batch's end in its last word, is written as zero:
// the layout's lanes past n stay zero and the next batch overwrites them); a bit-plane word is merged as
// (old & ~mask) | (ballot & mask) by one lane — one tile owns a (row, word) per launch and launches on the
// ctx stream are ordered. The one-shot kernels are left as they are (their code and resource use unchanged).
__global__ __launch_bounds__(256) void k_bincode_cw_tiles_at(const uint8_t* buf, uint64_t c0, uint64_t m, uint32_t d,
                                                             uint32_t L, uint32_t npad, uint32_t nw, uint4* d_cw_seed,
                                                             uint64_t* d_cw_bits, uint32_t* err) {
    __shared__ uint32_t st[64 * kBcRow];
    const uint32_t K = 2 * d;
    const uint64_t KB = 25 + 20ull * L, R = 8 + (uint64_t)K * KB;
    const uint32_t nlb = (L + kBcLevels - 1) / kBcLevels;
    const uint64_t nwb = bc_span_words(c0, m), w0 = bc_span_first_word(c0);
    const uint64_t tiles = nwb * K * nlb;
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t j = tile % nwb;
        const uint32_t kk = (uint32_t)((tile / nwb) % K);
        const uint32_t l0 = (uint32_t)(tile / (nwb * K)) * kBcLevels;
        const uint32_t nl = min((uint32_t)kBcLevels, L - l0);
        const BcWord sp = bc_span_word(c0, m, j);
        const uint64_t w = w0 + j;
        // stage (as k_bincode_cw_tiles): wave wv takes the word's lanes wv + 4 i, each from its own record
        uint32_t v[16][3];
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const uint32_t ln = wv + 4 * i;
            const bool in = (sp.lanes >> ln) & 1;
            const uint64_t rec = in ? (uint64_t)(sp.src0 + (int64_t)ln) : 0;
            const uint64_t s0 = 8 + rec * R + 8 + kk * KB + 25 + 20ull * l0;   // level l0's CorWord
            const uint64_t a0 = s0 & ~3ull;
            const uint32_t ndw = in ? (uint32_t)((s0 + 20ull * nl + 3 - a0) / 4) : 0u;   // <= kBcRow
            const uint32_t* src = reinterpret_cast<const uint32_t*>(buf + a0);
#pragma unroll
            for (int r = 0; r < 3; r++) {
                const uint32_t q = lane + 64 * r;
                v[i][r] = q < ndw ? src[q] : 0u;
            }
        }
#pragma unroll
        for (int i = 0; i < 16; i++)
#pragma unroll
            for (int r = 0; r < 3; r++) {
                const uint32_t q = lane + 64 * r;
                if (q < (uint32_t)kBcRow) st[(wv + 4 * i) * kBcRow + q] = v[i][r];
            }
        __syncthreads();
        const uint64_t c = w * 64 + lane;
        const bool in = (sp.lanes >> lane) & 1;
        const uint64_t mask = sp.lanes | sp.tail;
        const bool wr = (mask >> lane) & 1;
        const uint64_t rec = in ? (uint64_t)(sp.src0 + (int64_t)lane) : 0;
        const uint32_t sh = (uint32_t)((8 + rec * R + 8 + kk * KB + 25 + 20ull * l0) & 3) * 8;
        uint32_t bad = 0;
        for (uint32_t li = wv; li < nl; li += 4) {
            uint4 val = make_uint4(0, 0, 0, 0);
            uint32_t nib = 0;
            if (in) {
                const uint32_t* row = st + lane * kBcRow + 5 * li;   // 5 li + 5 < kBcRow
                uint32_t u[5];
#pragma unroll
                for (int k = 0; k < 5; k++) u[k] = __builtin_amdgcn_alignbit(row[k + 1], row[k], sh);
                val = make_uint4(u[0], u[1], u[2], u[3]);
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const uint32_t x = (u[4] >> (8 * b)) & 0xFFu;
                    bad |= x > 1 ? 1u : 0u;
                    nib |= (x & 1u) << b;
                }
            }
            const size_t rowi = (size_t)(l0 + li) * K + kk;
            if (wr) d_cw_seed[rowi * npad + c] = val;
            uint64_t q[4];
#pragma unroll
            for (int b = 0; b < 4; b++) q[b] = __ballot((nib >> b) & 1);
            if (lane == 0)
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    uint64_t* p = d_cw_bits + (rowi * 4 + b) * nw + w;
                    *p = ~mask ? ((*p & ~mask) | (q[b] & mask)) : q[b];
                }
        }
        if (bad) atomicOr(err, bad);
        __syncthreads();
    }
}

// level L of an appended batch: roots, key_idx and the records' length fields, one wave per (key, word)
__global__ void k_keys_from_bincode_at(const uint8_t* buf, uint64_t c0, uint64_t m, uint32_t d, uint32_t L,
                                       uint32_t npad, uint32_t nw, uint4* d_root, uint64_t* d_key_idx, uint32_t* err) {
    const uint32_t K = 2 * d;
    const uint64_t KB = 25 + 20ull * L, R = 8 + (uint64_t)K * KB;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wpb = blockDim.x >> 6;
    const uint64_t nwaves = (uint64_t)gridDim.x * wpb;
    const uint64_t nwb = bc_span_words(c0, m), w0 = bc_span_first_word(c0);
    const uint64_t items = nwb * K;
    for (uint64_t item = (uint64_t)blockIdx.x * wpb + wave_id_uniform(); item < items; item += nwaves) {
        const uint64_t j = item % nwb;
        const uint32_t kk = (uint32_t)(item / nwb);
        const BcWord sp = bc_span_word(c0, m, j);
        const uint64_t w = w0 + j, mask = sp.lanes | sp.tail;
        uint4 v = make_uint4(0, 0, 0, 0);
        uint32_t ki = 0, bad = 0;
        if ((sp.lanes >> lane) & 1) {
            const uint8_t* rec = buf + 8 + (uint64_t)(sp.src0 + (int64_t)lane) * R;
            const uint8_t* key = rec + 8 + (uint64_t)kk * KB;
            ki = key[0];
            bad |= ki > 1 ? 1u : 0u;
            v = load_seed(key + 1);
            bad |= load_u64_le(key + 17) != L ? 2u : 0u;
            if (kk == 0) bad |= load_u64_le(rec) != d ? 4u : 0u;
        }
        if ((mask >> lane) & 1) d_root[(size_t)kk * npad + w * 64 + lane] = v;
        const uint64_t q = __ballot(ki & 1u);
        if (lane == 0) {
            uint64_t* p = d_key_idx + (size_t)kk * nw + w;
            *p = ~mask ? ((*p & ~mask) | (q & mask)) : q;
        }
        if (bad) atomicOr(err, bad);
    }
}

hipError_t launch_keys_from_bincode_at(const uint8_t* buf, uint64_t c0, uint64_t m, uint32_t d, uint32_t L,
                                       uint32_t npad, uint32_t nw, uint4* d_cw_seed, uint64_t* d_cw_bits, uint4* d_root,
                                       uint64_t* d_key_idx, uint32_t* err, hipStream_t stream) {
    const uint64_t nwb = bc_span_words(c0, m);
    if (nwb == 0) return hipSuccess;
    if (bc_span_first_word(c0) + nwb > nw) return hipErrorInvalidValue;   // the caller sizes the layout first
    int dev = 0, cus = 256;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    const uint64_t tiles = nwb * 2 * d * ((L + kBcLevels - 1) / kBcLevels);
    if (tiles) {
        const uint64_t cap = (uint64_t)cus * 8;
        hipLaunchKernelGGL(k_bincode_cw_tiles_at, dim3((unsigned)(tiles < cap ? tiles : cap)), dim3(256), 0, stream, buf,
                           c0, m, d, L, npad, nw, d_cw_seed, d_cw_bits, err);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    uint64_t blocks = (nwb * 2 * d + 3) / 4;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(k_keys_from_bincode_at, dim3((unsigned)blocks), dim3(256), 0, stream, buf, c0, m, d, L, npad, nw,
                       d_root, d_key_idx, err);
    return hipGetLastError();
}

// rows of `width` elements from a layout of row pitch src_pitch into one of dst_pitch (elements): the key
// buffers' rows are [row][npad], so a change of capacity changes every row's pitch
template <class T>
__global__ void k_repitch(const T* src, T* dst, uint64_t rows, uint64_t width, uint64_t src_pitch, uint64_t dst_pitch) {
    const uint64_t total = rows * width;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = i / width, x = i % width;
        dst[r * dst_pitch + x] = src[r * src_pitch + x];
    }
}

template <class T>
static hipError_t launch_repitch(const T* src, T* dst, uint64_t rows, uint64_t width, uint64_t src_pitch,
                                 uint64_t dst_pitch, hipStream_t stream) {
    const uint64_t total = rows * width;
    if (total == 0) return hipSuccess;
    uint64_t blocks = (total + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(k_repitch<T>, dim3((unsigned)blocks), dim3(256), 0, stream, src, dst, rows, width, src_pitch,
                       dst_pitch);
    return hipGetLastError();
}

hipError_t launch_repitch_seeds(const uint4* src, uint4* dst, uint64_t rows, uint64_t width, uint64_t src_pitch,
                                uint64_t dst_pitch, hipStream_t stream) {
    return launch_repitch(src, dst, rows, width, src_pitch, dst_pitch, stream);
}

hipError_t launch_repitch_words(const uint64_t* src, uint64_t* dst, uint64_t rows, uint64_t width, uint64_t src_pitch,
                                uint64_t dst_pitch, hipStream_t stream) {
    return launch_repitch(src, dst, rows, width, src_pitch, dst_pitch, stream);
}

hipError_t launch_keys_from_aos(const uint8_t* key_idx, const uint8_t* root_seed, const uint8_t* cw_seed,
                                const uint8_t* cw_bits, uint64_t n, uint32_t K, uint32_t L, uint32_t npad, uint32_t nw,
                                uint4* d_cw_seed, uint64_t* d_cw_bits, uint4* d_root, uint64_t* d_key_idx,
                                hipStream_t stream) {
    const uint64_t items = (uint64_t)((L + 7) / 8 + 1) * K * nw;
    uint64_t blocks = (items + 3) / 4;
    if (blocks > 8192) blocks = 8192;
    if (blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(k_keys_from_aos, dim3((unsigned)blocks), dim3(256), 0, stream, key_idx, root_seed, cw_seed,
                       cw_bits, n, K, L, npad, nw, d_cw_seed, d_cw_bits, d_root, d_key_idx);
    return hipGetLastError();
}

}  // namespace fhh
