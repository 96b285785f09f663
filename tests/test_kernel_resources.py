"""Register budget of the hot kernel (CPU, hipcc cross-compile): the default k_expand variant
(kDefaultVariant = 52 in csrc/fhh_host.cpp = X(52, PAIR, MW, NTL all true, ...) in
csrc/fhh_kernels.hip, 1024 threads) must not spill and must keep 4 waves per SIMD.
A spill once crept in through extra item-decode state and cost 4-8 %."""
from kernel_usage import resource_usage

DEFAULT_EXPAND = "_ZN3fhh8k_expandILb1ELb1ELb1EEEvNS_12ExpandLaunchEPj"


def test_default_expand_variant_does_not_spill():
    u = resource_usage("fhh_kernels.hip")
    assert DEFAULT_EXPAND in u, "default k_expand instantiation not found (variant table changed?)"
    k = u[DEFAULT_EXPAND]
    assert k["ScratchSize [bytes/lane]"] == "0", k
    assert k["VGPRs Spill"] == "0", k
    assert int(k["Occupancy [waves/SIMD]"]) >= 4, k
    # 128 KiB of T-tables + the per-block drained mask of the work heads
    assert int(k["LDS Size [bytes/block]"]) == 131072 + 4, k


# every mode of both hashes (0 plain OT, 1 labels C-OT, 2 FE share C-OT, 3 FieldElm share C-OT)
OT_HASH_ROWS = tuple(f"_ZN3fhh19k_ot_{k}_hash_rowsILi{m}EEEvNS_6OtArgsE" for k in ("send", "recv") for m in range(4))


def test_ot_hash_rows_do_not_spill():
    """The transpose-fused OT hashes keep a lane's 32 tile words beside the AES; an unrolled
    round loop once spilled ~90 VGPRs. 160 KiB of LDS: tables + staging."""
    u = resource_usage("fhh_ot.hip")
    for name in OT_HASH_ROWS:
        assert name in u, f"{name} not found"
        k = u[name]
        assert k["ScratchSize [bytes/lane]"] == "0", (name, k)
        assert int(k["Occupancy [waves/SIMD]"]) >= 4, (name, k)
        assert int(k["LDS Size [bytes/block]"]) == 163840, (name, k)


def test_fe_sketch_kernels_resources():
    """The shipped FE sketch kernels (fhh_sketch.hip): the fused k_sketch_fe<KPW, SCHED = 2> and the producer /
    consumer k_sketch_fe_pc<KPW, 3> at KPW = 1, 2, 4, 8 keys per wave. 1024 threads at 4 waves per SIMD leave
    128 VGPRs; the only scratch is the out-of-line sequential fallback's frame. LDS: 128 KiB of tables + the
    fused kernel's per-key round keys (16 waves x KPW keys x 11 x 16 B) or the producer / consumer hand-over
    buffer (8 pairs x 3 blocks x 64 lanes x 16 B). Beside them k_sketch_fe may be built only in the two forms
    that the suite's r01-256 / otf-1024 cases run, <4, 0> (r01) and <8, 1> (on the fly), and in no other."""
    u = resource_usage("fhh_sketch.hip")
    lds = {f"_ZN3fhh11k_sketch_feILi{kpw}ELi2EEEvNS_10SketchArgsE": 131072 + 16 * kpw * 176 for kpw in (1, 2, 4, 8)}
    assert sorted(lds.values()) == [133888, 136704, 142336, 153600]
    lds.update({f"_ZN3fhh14k_sketch_fe_pcILi{kpw}ELi3EEEvNS_10SketchArgsE": 131072 + 24576 for kpw in (1, 2, 4, 8)})
    for name, want in lds.items():
        assert name in u, f"{name} not found"
        k = u[name]
        assert k["VGPRs Spill"] == "0", (name, k)
        assert int(k["ScratchSize [bytes/lane]"]) <= 32, (name, k)
        assert int(k["Occupancy [waves/SIMD]"]) >= 4, (name, k)
        assert int(k["LDS Size [bytes/block]"]) == want, (name, k)
    # (k_sketch_fe255 and k_sketch_fe_pc mangle to other prefixes: 14k_sketch_fe...)
    others = {n for n in u if n.startswith("_ZN3fhh11k_sketch_feI") and n not in lds}
    assert others <= {"_ZN3fhh11k_sketch_feILi4ELi0EEEvNS_10SketchArgsE",
                      "_ZN3fhh11k_sketch_feILi8ELi1EEEvNS_10SketchArgsE"}, others


def test_gc_and_ot_expand_kernels_do_not_spill():
    """k_gc_garble / k_gc_eval at every share-string width b = 1..8, the garbled-table kernels and both
    OT expands (ChaCha12 since r06) stay in registers at >= 4 waves per SIMD."""
    u = resource_usage("fhh_gc.hip")
    # both garblers (the ideal-OT one, the r05 one on the labels C-OT's zero labels with the garbler's
    # string folded in) and both evaluator forms
    names = [f"_ZN3fhh11k_gc_garbleILi{b}EEEvNS_6GcArgsE" for b in range(1, 9)]
    names += [f"_ZN3fhh15k_gc_garble_cotILi{b}EEEvNS_6GcArgsE" for b in range(1, 9)]
    names += [f"_ZN3fhh9k_gc_evalILi{b}ELb{f}EEEvNS_6GcArgsE" for b in range(1, 9) for f in (0, 1)]
    # r05d: the garbled table on the row-major labels, b = 3, 4, shares in FE (0) and in Z_2^32 (1)
    names += [f"_ZN3fhh11k_gt_garbleILi{b}ELb{r}EEEvNS_6GcArgsE" for b in (3, 4) for r in (0, 1)]
    names += [f"_ZN3fhh9k_gt_evalILi{b}ELb{r}EEEvNS_6GcArgsE" for b in (3, 4) for r in (0, 1)]
    # (b <= 2 is tile-major for every caller: no row-major kernel exists there, test_table_ring32_wide.py)
    # r06: the table kernels on the labels OT's tile-major Q / T (b <= 2)
    # (r06: FE and Z_2^32 shares as separate instantiations)
    names += [f"_ZN3fhh14k_gt_garble_tmILi{b}ELb{r}EEEvNS_6GcArgsE" for b in (1, 2) for r in (0, 1)
              if (b, r) != (2, 1)]
    names += [f"_ZN3fhh12k_gt_eval_tmILi{b}EEEvNS_6GcArgsE" for b in (1, 2)]
    u.update(resource_usage("fhh_ot.hip"))
    # r06: the ChaCha12 row-PRG expands (no LDS), and the labels OT's row transpose (mode 4, r05b)
    names += ["_ZN3fhh19k_ot_recv_expand_ccENS_6OtArgsE", "_ZN3fhh19k_ot_send_expand_ccENS_6OtArgsE",
              "_ZN3fhh13k_ot_rows_outENS_6OtArgsEi"]
    for name in names:
        assert name in u, f"{name} not found"
        k = u[name]
        assert k["ScratchSize [bytes/lane]"] == "0", (name, k)
        assert k["VGPRs Spill"] == "0", (name, k)
        assert int(k["Occupancy [waves/SIMD]"]) >= 4, (name, k)
    # r06: the b = 2 garbler's Z_2^32 instantiation keeps the FE code beside a runtime test (RING && a.ring32):
    # compiled that way it spills one VGPR and still ran ~11 % faster than a Z_2^32-only body (2282 vs 2553 us
    # per launch, profiles/r06/ring32/); allow that one
    k = u["_ZN3fhh14k_gt_garble_tmILi2ELb1EEEvNS_6GcArgsE"]
    assert int(k["VGPRs Spill"]) <= 1 and int(k["Occupancy [waves/SIMD]"]) >= 4, k
    # r06 SoftSpoken (k = 2, 4): the GGM trees and both expands stay in registers; k = 4 keeps 4 / 3 row sums
    # of 16 words beside two ChaCha blocks (occupancy 2-3 at 256-thread workgroups, VALU-bound)
    for name in [f"_ZN3fhh{len(f'k_ss_{r}')}k_ss_{r}ILi{k}EEEvNS_6OtArgsE" for r in ("ggm", "recv_expand", "send_expand")
                 for k in (2, 4)]:
        assert name in u, f"{name} not found"
        k = u[name]
        assert k["ScratchSize [bytes/lane]"] == "0", (name, k)
        assert k["VGPRs Spill"] == "0", (name, k)
        assert int(k["Occupancy [waves/SIMD]"]) >= 2, (name, k)
