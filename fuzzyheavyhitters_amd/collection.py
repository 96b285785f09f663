"""Python mirror of the reference's `KeyCollection<FE, FieldElm>` (src/collect.rs:28-1030),
backed by the HIP engine in libfhh.so. Same method names and argument meaning; errors raise
FhhError where the reference panics.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from ._lib import (FHH_BALL_BITS, FHH_BALL_COORDS, FhhAuditReport, FhhBallSrc, FhhError, FhhStats, check, lib, ptr, u32p,
                   u64p)
from .fields import FE255_P, FE_P, limbs10_to_int, int_to_limbs


@dataclass
class Result:
    """collect.rs:39-43: `Result<T> { path: Vec<Vec<bool>>, value: T }`."""
    path: list      # d lists of bools
    value: int      # unreduced FieldElm sum as int (or count in plaintext-count harness mode)


def _keep_bytes(keep) -> np.ndarray:
    """A keep mask as the uint8 bytes the C ABI takes: bools, or integers passed on as they are (the library
    refuses a byte other than 0/1). Other dtypes, and integers outside a byte, are refused here: a cast would
    turn 0.5 or 256 into 0 silently."""
    a = np.asarray(keep)
    if a.dtype != np.bool_ and not np.issubdtype(a.dtype, np.integer):
        raise FhhError(f"keep mask of dtype {a.dtype}: bools or integers 0/1 expected")
    if a.dtype != np.bool_ and a.size and (a.min() < 0 or a.max() > 255):
        raise FhhError("keep mask: an entry is not 0 or 1")
    return np.ascontiguousarray(a.astype(np.uint8)).reshape(-1)


def _device_mask(keep, n, n_rows, row_stride):
    """(pointer, n, n_rows, row_stride) of a keep mask in device memory: a torch.uint8 tensor [n] or [rows, n] on a
    GPU, or an integer device pointer with the sizes given. What the C ABI cannot see is refused here: a dtype
    other than uint8, a CPU tensor, a column stride other than 1, rows that overlap."""
    if isinstance(keep, (int, np.integer)):
        if n is None:
            raise FhhError("keep mask given as a device pointer: n is required")
        if n_rows > 1 and row_stride is None:
            raise FhhError("keep mask given as a device pointer with several rows: row_stride is required")
        return ctypes.c_void_p(int(keep)), int(n), int(n_rows), int(n if row_stride is None else row_stride)
    if not (hasattr(keep, "data_ptr") and hasattr(keep, "is_cuda")):
        raise FhhError("keep mask: a torch.uint8 tensor on the GPU or an integer device pointer expected "
                       "(a host mask goes to retain_clients)")
    import torch
    if keep.dtype != torch.uint8:
        raise FhhError(f"keep mask of dtype {keep.dtype}: torch.uint8 expected")
    if not keep.is_cuda:
        raise FhhError("keep mask on the CPU: retain_clients takes host masks")
    if keep.dim() not in (1, 2):
        raise FhhError(f"keep mask of shape {tuple(keep.shape)}: [n] or [rows, n] expected")
    rows, cols = (1, keep.shape[0]) if keep.dim() == 1 else keep.shape
    if cols > 1 and keep.stride(-1) != 1:
        raise FhhError("keep mask: the clients of a row must be contiguous (column stride 1)")
    stride = cols if keep.dim() == 1 or rows == 1 else keep.stride(0)
    if rows > 1 and stride < cols:
        raise FhhError("keep mask: row stride below the row length")
    torch.cuda.synchronize(keep.device)   # the library reads on its own stream: torch's writes must be complete
    return ctypes.c_void_p(keep.data_ptr()), int(cols), int(rows), int(stride)


class KeyAuditError(FhhError):
    """Keys that do not mean what their points say (`leader.add_fuzzy_keys(audit=True)`): `report` is the audit's
    report (`KeyCollection.audit_keys_ball`), `ok` its per-client bytes, `first` the population index of the audited
    chunk's client 0."""

    def __init__(self, report: dict, ok: np.ndarray, first: int = 0):
        self.report, self.ok, self.first = report, ok, first
        super().__init__(f"key audit: {report['n_bad_clients']} of {ok.size} clients from client {first} on fail; first "
                         f"client {report['first_client']} dim {report['first_dim']} side {report['first_side']} probe "
                         f"{report['first_probe']} level {report['first_level']}: got {report['got']}, expected "
                         f"{report['expected']}")


def _audit_report(rep: FhhAuditReport, c: "KeyCollection") -> dict:
    """fhh_audit_report as a dict (first_client None when every client is ok), with the diagnostics of the call:
    the kernel's time and the walks whose seeds diverged (fhh_audit_timing, fhh_audit_seed_check)."""
    out = {name: int(getattr(rep, name)) for name, _ in FhhAuditReport._fields_}
    if out["first_client"] == 2 ** 64 - 1:
        out["first_client"] = None
    ms, div = ctypes.c_double(), ctypes.c_uint64()
    check(lib().fhh_audit_timing(c.handle, ctypes.byref(ms)), c.handle)
    check(lib().fhh_audit_seed_check(c.handle, ctypes.byref(div)), c.handle)
    out["kernel_ms"] = ms.value
    out["seed_diverged"] = int(div.value)
    return out


class KeyCollection:
    """One server's key collection (collect.rs:45-1030) on one GPU, or — with `devices` — one
    collection whose clients are sharded over several GPUs (fhh_create_multi: contiguous ranges
    of 64-client words, per-child partials reduced over an in-process RCCL communicator, or on
    the host when a device repeats). The methods are the same either way."""

    def __init__(self, depth: int, n_dims: int, device: int = 0, devices=None):
        # KeyCollection::new(seed, depth) (collect.rs:51-60)
        self.depth = depth
        self.n_dims = n_dims
        self.device = device if devices is None else int(devices[0])
        self.devices = None if devices is None else [int(x) for x in devices]
        self._owner = None
        h = ctypes.c_void_p()
        if devices is None:
            check(lib().fhh_create(ctypes.byref(h), depth, n_dims, device))
        else:
            arr = (ctypes.c_int * len(self.devices))(*self.devices)
            check(lib().fhh_create_multi(ctypes.byref(h), depth, n_dims, arr, len(self.devices)))
        self._h = h

    @classmethod
    def _borrowed(cls, owner: "KeyCollection", handle, device: int):
        """A shard's ctx, owned by `owner` (never destroyed through this object)."""
        kc = cls.__new__(cls)
        kc.depth, kc.n_dims, kc.device, kc.devices = owner.depth, owner.n_dims, device, None
        kc._owner = owner
        kc._h = handle
        return kc

    def shard_info(self):
        """[(device, client_base, n_clients)] per shard and the reduction ("none" / "host" / "rccl")."""
        from ._lib import FHH_REDUCE_NAMES
        out = []
        ns, dev, red = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        base, cnt = ctypes.c_uint64(), ctypes.c_uint64()
        k = 0
        while True:
            self._chk(lib().fhh_shard_info(self._h, k, ctypes.byref(ns), ctypes.byref(dev), ctypes.byref(base),
                                           ctypes.byref(cnt), ctypes.byref(red)))
            out.append((dev.value, base.value, cnt.value))
            k += 1
            if k >= ns.value:
                break
        return out, FHH_REDUCE_NAMES[red.value]

    def shard(self, k: int) -> "KeyCollection":
        """Shard k's one-GPU collection (per-shard calls: the two-party GC + OT, fhh_gb_* / fhh_ev_*)."""
        h = ctypes.c_void_p()
        self._chk(lib().fhh_shard_ctx(self._h, k, ctypes.byref(h)))
        if h.value == (self._h.value if isinstance(self._h, ctypes.c_void_p) else self._h):
            return self
        return KeyCollection._borrowed(self, h, self.shard_info()[0][k][0])

    @property
    def handle(self):
        return self._h

    def close(self):
        if getattr(self, "_owner", None) is not None:   # a borrowed shard ctx
            self._h = None
            return
        if getattr(self, "_h", None):
            lib().fhh_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        check(rc, self._h)

    # ---- keys -----------------------------------------------------------------------
    def add_keys(self, key_idx: np.ndarray, root_seed: np.ndarray, cw_seed: np.ndarray, cw_bits: np.ndarray):
        """Batched `add_key` (collect.rs:62-65). Shapes [n][d][2], [n][d][2][16],
        [n][d][2][L][16], [n][d][2][L] (uint8)."""
        n = key_idx.shape[0]
        d, L = self.n_dims, self.depth
        if key_idx.shape != (n, d, 2) or root_seed.shape != (n, d, 2, 16) or cw_seed.shape != (n, d, 2, L, 16) \
                or cw_bits.shape != (n, d, 2, L):
            raise FhhError("add_keys: shape mismatch")
        a = [np.ascontiguousarray(x, np.uint8) for x in (key_idx, root_seed, cw_seed, cw_bits)]
        self._chk(lib().fhh_add_keys(self._h, n, *[ptr(x) for x in a]))

    def add_keys_bincode(self, request: bytes):
        """The `add_keys` RPC payload (rpc.rs:12-15: `Vec<Vec<(ibDCFKey, ibDCFKey)>>` in bincode
        legacy encoding), decoded on the GPU straight into the device layout."""
        buf = np.frombuffer(bytes(request), np.uint8) if not isinstance(request, np.ndarray) else \
            np.ascontiguousarray(request, np.uint8)
        self._chk(lib().fhh_add_keys_bincode(self._h, ptr(buf), buf.size))

    def reserve_clients(self, n: int):
        """Size the device key layout for n clients before `add_keys_bincode_append`. Optional on one
        GPU (a reservation of the final count saves the growth and compaction copies), required with
        `devices` (the shards' client ranges depend on the total)."""
        self._chk(lib().fhh_reserve_clients(self._h, n))

    def add_keys_bincode_append(self, request: bytes):
        """One `add_keys` RPC of the leader's stream of batches (leader.rs:391-415; the framing of
        `add_keys_bincode`): its clients are appended after those the collection holds and decoded on
        the GPU into their place. A malformed batch raises and leaves the collection as it was."""
        buf = np.frombuffer(bytes(request), np.uint8) if not isinstance(request, np.ndarray) else \
            np.ascontiguousarray(request, np.uint8)
        self._chk(lib().fhh_add_keys_bincode_append(self._h, ptr(buf), buf.size))

    def num_clients(self) -> int:
        n = ctypes.c_uint64()
        self._chk(lib().fhh_num_clients(self._h, ctypes.byref(n)))
        return n.value

    def export_keys(self):
        n, d, L = self.num_clients(), self.n_dims, self.depth
        ki = np.zeros((n, d, 2), np.uint8)
        rs = np.zeros((n, d, 2, 16), np.uint8)
        cs = np.zeros((n, d, 2, L, 16), np.uint8)
        cb = np.zeros((n, d, 2, L), np.uint8)
        self._chk(lib().fhh_export_keys(self._h, ptr(ki), ptr(rs), ptr(cs), ptr(cb)))
        return ki, rs, cs, cb

    def export_keys_bincode(self, first: int = 0, count: int | None = None, batch: int = 0) -> np.ndarray:
        """Clients [first, first + count) of the device keys as consecutive `add_keys` RPC payloads of
        `batch` clients each (0: one request; leader.rs:391-415 sends addkey_batch_size = 100), serialized
        on the GPU: what `add_keys_bincode` / `add_keys_bincode_append` take. One uint8 array holding the
        requests back to back; `workload.split_add_keys_requests` cuts it. count = None: up to the last
        client."""
        if count is None:
            count = self.num_clients() - first
        need = ctypes.c_uint64()
        self._chk(lib().fhh_bincode_request_bytes(self.n_dims, self.depth, count, batch, ctypes.byref(need)))
        out = np.empty(need.value, np.uint8)
        got = ctypes.c_uint64()
        self._chk(lib().fhh_export_keys_bincode(self._h, first, count, batch, ptr(out), out.size, ctypes.byref(got)))
        assert got.value == out.size
        return out

    def audit_keys_ball(self, other: "KeyCollection", points: np.ndarray, ball: int, form: str = "bits"):
        """Do the keys mean what the points say (fhh_audit_keys_ball)? self holds server 0's keys, `other` server
        1's, of the clients whose `points` (in `gen_keys_ball`'s layout for `form`) and `ball` made them. Both
        servers' keys of every client are evaluated on the GPU at the probes l - 1, l, a, r, r + 1 of each dim
        and, after every level, the reconstructed bit is compared with the interval rule. Returns (ok, report):
        ok uint8 [n], 1 for a client whose comparisons all hold; report a dict of fhh_audit_report's fields
        (first_client None when all are ok) plus kernel_ms and seed_diverged. The collections are otherwise
        unchanged: the call may come between the levels of a crawl. A failed audit is a result, not an error."""
        src, n, keep = _ball_src(points, ball, form, self.n_dims, self.depth, None, bytes(32), 0)
        ok = np.zeros(n, np.uint8)
        rep = FhhAuditReport()
        self._chk(lib().fhh_audit_keys_ball(self._h, other.handle, n, ctypes.byref(src), ptr(ok) if n else None,
                                            ctypes.byref(rep)))
        del keep
        return ok, _audit_report(rep, self)

    def audit_keys_ball_device(self, other: "KeyCollection", points: np.ndarray, ball: int, form: str = "bits"):
        """`audit_keys_ball` with the ok bytes left in device memory (fhh_audit_keys_ball_device; one-GPU
        collections only): (ok, report) with ok a torch.uint8 tensor [n] on this collection's GPU, a copy of the
        library's buffer made on the device, usable as a mask (row) of `retain_clients_device`."""
        import torch
        src, n, keep = _ball_src(points, ball, form, self.n_dims, self.depth, None, bytes(32), 0)
        p = ctypes.c_void_p()
        rep = FhhAuditReport()
        self._chk(lib().fhh_audit_keys_ball_device(self._h, other.handle, n, ctypes.byref(src), ctypes.byref(p),
                                                   ctypes.byref(rep)))
        del keep
        ok = torch.empty(n, dtype=torch.uint8, device=f"cuda:{self.device}")
        torch.cuda.synchronize(self.device)
        check(lib().fhh_memcpy_device(self.device, ctypes.c_void_p(ok.data_ptr()), p, n))
        return ok, _audit_report(rep, self)

    def retain_clients(self, keep):
        """`apply_sketch_results` (main.rs:68-69): drop the clients whose keep entry is false (fhh_retain_clients).
        Afterwards this is a collection of the survivors, in their old order, at the same frontier; both servers
        call it with the same mask. keep: one 0/1 (or bool) entry per client."""
        k = _keep_bytes(keep)
        self._chk(lib().fhh_retain_clients(self._h, ptr(k) if k.size else None, k.size))

    @staticmethod
    def retain_plan(keep):
        """fhh_retain_plan (host arithmetic): (n_kept, src) with src[k] = the old index of the k-th survivor."""
        k = _keep_bytes(keep)
        nk = ctypes.c_uint64()
        src = np.zeros(max(k.size, 1), np.uint32)
        check(lib().fhh_retain_plan(ptr(k) if k.size else None, k.size, ctypes.byref(nk), ptr(src, u32p)))
        return int(nk.value), src[: nk.value].copy()

    def retain_clients_device(self, keep, n=None, n_rows=1, row_stride=None) -> int:
        """`retain_clients` with the mask in device memory (fhh_retain_clients_device): the mask never crosses to
        the host. keep: a CUDA/HIP torch.uint8 tensor [n] or [rows, n] (row stride >= n, unit column stride), or an
        integer device pointer with n / n_rows / row_stride given. A client survives iff its byte is 1 in every
        row. The tensor's device is synchronised first: the library reads the mask on its own stream. Returns the
        number of survivors."""
        p, n, n_rows, row_stride = _device_mask(keep, n, n_rows, row_stride)
        nk = ctypes.c_uint64()
        self._chk(lib().fhh_retain_clients_device(self._h, p, n, n_rows, row_stride, ctypes.byref(nk)))
        return int(nk.value)

    def retain_plan_device(self, keep, n=None, n_rows=1, row_stride=None):
        """fhh_retain_plan_device (the survivor-list kernels alone, on this collection's device and stream): (n_kept,
        src) as `retain_plan` gives them, of a mask as `retain_clients_device` takes it."""
        p, n, n_rows, row_stride = _device_mask(keep, n, n_rows, row_stride)
        nk = ctypes.c_uint64()
        src = np.zeros(max(n, 1), np.uint32)
        self._chk(lib().fhh_retain_plan_device(self._h, p, n, n_rows, row_stride, ctypes.byref(nk), ptr(src, u32p)))
        return int(nk.value), src[: nk.value].copy()

    def retain_mask_timing(self):
        """(words + scan ms, emit ms) of the survivor-list kernels' last runs on this collection (HIP events)."""
        ms = (ctypes.c_double * 2)()
        self._chk(lib().fhh_retain_mask_timing(self._h, ms))
        return ms[0], ms[1]

    def retain_timing(self):
        """((column ms, plane ms), (column bytes, plane bytes)) of the last retain_clients that ran its kernels."""
        ms = (ctypes.c_double * 2)()
        by = (ctypes.c_uint64 * 2)()
        self._chk(lib().fhh_retain_timing(self._h, ms, by))
        return (ms[0], ms[1]), (int(by[0]), int(by[1]))

    def join_clients_bincode(self, request: bytes):
        """One `add_keys` request (the framing of `add_keys_bincode_append`) whose clients join a crawl in progress
        (fhh_join_clients_bincode): the collection must have a frontier (after `tree_init`, `tree_init_at`, a prune
        or `sim_crawl`). Afterwards it holds the old clients followed by the joiners, at the same frontier, as a
        fresh collection of all of them brought there with `tree_init_at(frontier_paths())` would; only the joiners'
        keys are walked. Both servers call it with their halves of the same batch. A refused batch raises and leaves
        the collection as it was."""
        buf = np.frombuffer(bytes(request), np.uint8) if not isinstance(request, np.ndarray) else \
            np.ascontiguousarray(request, np.uint8)
        self._chk(lib().fhh_join_clients_bincode(self._h, ptr(buf) if buf.size else None, buf.size))

    @staticmethod
    def join_plan(n_dims: int, depth: int, n: int, m: int, n_unique, grid_blocks: int) -> dict:
        """fhh_join_plan (host arithmetic, no GPU): the walk of m clients joining n at a frontier of `depth` levels
        with n_unique[j] live entries in dim j, on at most grid_blocks workgroups — first_word, first_mask, words,
        new_nw, items, waves, trips, last_trip_items, aes_blocks."""
        names = ("first_word", "first_mask", "words", "new_nw", "items", "waves", "trips", "last_trip_items",
                 "aes_blocks")
        nu = np.ascontiguousarray(n_unique, np.uint32).reshape(-1)
        v = [ctypes.c_uint64() for _ in names]
        check(lib().fhh_join_plan(n_dims, depth, n, m, ptr(nu, u32p) if nu.size else None, grid_blocks,
                                  *[ctypes.byref(x) for x in v]))
        return {k: int(x.value) for k, x in zip(names, v)}

    def join_timing(self):
        """((re-pitch ms, decode ms, walk ms), re-pitch bytes read plus written) of the last join_clients_bincode
        that ran its kernels here (HIP events)."""
        ms = (ctypes.c_double * 3)()
        by = (ctypes.c_uint64 * 1)()
        self._chk(lib().fhh_join_timing(self._h, ms, by))
        return (ms[0], ms[1], ms[2]), int(by[0])

    def set_client_base(self, base: int):
        self._chk(lib().fhh_set_client_base(self._h, base))

    # ---- crawl ----------------------------------------------------------------------
    def tree_init(self):
        self._chk(lib().fhh_tree_init(self._h))

    def _paths_array(self, paths) -> np.ndarray:
        """A frontier as uint8 [F][d][depth]: an array of that shape, or nodes given as d tuples of direction bits
        (what `workload.plaintext_crawl` returns; one node `((), ...)` of empty tuples is the root)."""
        a = np.asarray(paths if isinstance(paths, np.ndarray) else [[list(p) for p in node] for node in paths])
        if a.ndim == 2 and a.shape[1] == self.n_dims and a.size == 0:
            a = a.reshape(a.shape[0], self.n_dims, 0)
        if a.ndim != 3 or a.shape[1] != self.n_dims:
            raise FhhError(f"paths must be [F][{self.n_dims}][depth], got shape {a.shape}")
        return np.ascontiguousarray(a, np.uint8)

    def tree_init_at(self, paths):
        """`tree_init` at a given frontier instead of the root (fhh_tree_init_at): node k of the frontier is
        paths[k], the next `tree_crawl` runs level `depth`. A checkpoint taken with `frontier_paths` is restored
        this way; candidate prefixes are counted by seeding their parents and crawling once."""
        a = self._paths_array(paths)
        self._chk(lib().fhh_tree_init_at(self._h, a.shape[0], a.shape[2], ptr(a) if a.size else None))

    def frontier_paths(self) -> np.ndarray:
        """uint8 [F][d][depth]: the paths of the nodes `frontier_size` counts in its first value (after an
        unpruned `tree_crawl` the pending children, in `export_states`' order)."""
        nn, dep = ctypes.c_uint64(), ctypes.c_uint32()
        self._chk(lib().fhh_frontier_paths(self._h, ctypes.byref(nn), ctypes.byref(dep), None))
        out = np.zeros((int(nn.value), self.n_dims, int(dep.value)), np.uint8)
        if out.size:
            self._chk(lib().fhh_frontier_paths(self._h, ctypes.byref(nn), ctypes.byref(dep), ptr(out)))
        return out

    @staticmethod
    def frontier_plan(paths: np.ndarray):
        """fhh_frontier_plan (host arithmetic): (n_unique [d], pos [F][d]) of paths uint8 [F][d][depth]."""
        a = np.ascontiguousarray(paths, np.uint8)
        if a.ndim != 3:
            raise FhhError(f"paths must be [F][d][depth], got shape {a.shape}")
        F, d, depth = a.shape
        nu = np.zeros(max(d, 1), np.uint32)
        pos = np.zeros((F, d), np.uint32)
        check(lib().fhh_frontier_plan(d, depth, F, ptr(a) if a.size else None, ptr(nu, u32p),
                                      ptr(pos, u32p) if pos.size else None))
        return nu[:d], pos

    def _crawl(self, fn, share_planes: bool):
        nch = ctypes.c_uint64()
        if not share_planes:
            self._chk(fn(self._h, ctypes.byref(nch), None))
            return int(nch.value), None
        # query size: frontier size * 2^d
        f = ctypes.c_uint64()
        self._chk(lib().fhh_frontier_size(self._h, ctypes.byref(f), None))
        n = self.num_clients()
        nw = (n + 63) // 64
        # a pending (unpruned) crawl becomes the frontier first; size it generously
        C = int(f.value) << self.n_dims
        planes = np.zeros((C, 2 * self.n_dims, nw), np.uint64)
        self._chk(fn(self._h, ctypes.byref(nch), ptr(planes, u64p)))
        return int(nch.value), planes[: nch.value]

    def tree_crawl(self, share_planes: bool = False):
        """Expansion half of `tree_crawl` (collect.rs:370-418). Returns (C, planes|None);
        planes[c][k][w] bit (client % 64) = share bit k of (child c, client)."""
        return self._crawl(lib().fhh_tree_crawl, share_planes)

    def tree_crawl_last(self, share_planes: bool = False):
        return self._crawl(lib().fhh_tree_crawl_last, share_planes)

    def node_sums_fe(self, vals: np.ndarray) -> np.ndarray:
        """collect.rs:487-501: vals [C][n] u64 -> canonical FE sums [C]."""
        v = np.ascontiguousarray(vals, np.uint64)
        out = np.zeros(v.shape[0], np.uint64)
        self._chk(lib().fhh_node_sums_fe(self._h, ptr(v, u64p), ptr(out, u64p)))
        return out

    def node_sums_fe_device(self, vals_dev, ld: int, C: int, fmt: int = 0) -> np.ndarray:
        """collect.rs:487-501 on OT outputs already in device memory (no host round trip):
        vals_dev = one device pointer (int) per shard, rows [C][ld] (C = the pending crawl's
        children; ld = the row pitch in values, at least the shard's client count, 0 = "this
        ctx's n": each shard's own client count); fmt FHH_VALS_FE_U64 / FHH_VALS_FE_BLOCK.
        Returns canonical FE sums [C]."""
        ptrs = (ctypes.c_void_p * len(vals_dev))(*[int(p) for p in vals_dev])
        out = np.zeros(max(C, 1), np.uint64)
        self._chk(lib().fhh_node_sums_fe_device(self._h, ptrs, ld, fmt, ptr(out, u64p)))
        return out[:C]

    def node_sums_fe255_device(self, vals_dev, ld: int, C: int, fmt: int = 3):
        """collect.rs:891-905 on device-resident FieldElm OT outputs (FHH_VALS_FE255_LIMBS /
        FHH_VALS_FE255_BLOCKPAIR), one device pointer per shard, rows [C][ld] with ld as in
        `node_sums_fe_device` (0 = "this ctx's n") -> (unreduced ints, canonical ints)."""
        ptrs = (ctypes.c_void_p * len(vals_dev))(*[int(p) for p in vals_dev])
        unr = np.zeros((max(C, 1), 10), np.uint32)
        can = np.zeros((max(C, 1), 8), np.uint32)
        self._chk(lib().fhh_node_sums_fe255_device(self._h, ptrs, ld, fmt, ptr(unr, u32p), ptr(can, u32p)))
        return [limbs10_to_int(r) for r in unr[:C]], [limbs10_to_int(r) for r in can[:C]]

    def node_sums_fe255(self, vals: np.ndarray):
        """collect.rs:891-905: vals [C][n][8] u32 LE limbs -> (unreduced ints, canonical ints)."""
        v = np.ascontiguousarray(vals, np.uint32)
        C = v.shape[0]
        unr = np.zeros((C, 10), np.uint32)
        can = np.zeros((C, 8), np.uint32)
        self._chk(lib().fhh_node_sums_fe255(self._h, ptr(v, u32p), ptr(unr, u32p), ptr(can, u32p)))
        return [limbs10_to_int(r) for r in unr], [limbs10_to_int(r) for r in can]

    def tree_prune(self, keep):
        k = np.ascontiguousarray(np.asarray(keep, bool).astype(np.uint8))
        self._chk(lib().fhh_tree_prune(self._h, ptr(k), k.size))

    def tree_prune_last(self, keep):
        k = np.ascontiguousarray(np.asarray(keep, bool).astype(np.uint8))
        self._chk(lib().fhh_tree_prune_last(self._h, ptr(k), k.size))

    def frontier_size(self):
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        self._chk(lib().fhh_frontier_size(self._h, ctypes.byref(a), ctypes.byref(b)))
        return int(a.value), int(b.value)

    def final_shares(self):
        """collect.rs:993-1005 -> list of Result(path, value)."""
        nf, lv = ctypes.c_uint64(), ctypes.c_uint32()
        self._chk(lib().fhh_final_shares(self._h, ctypes.byref(nf), ctypes.byref(lv), None, None))
        F, L = int(nf.value), int(lv.value)
        paths = np.zeros((F, self.n_dims, max(L, 1)), np.uint8)
        vals = np.zeros((F, 10), np.uint32)
        if F:
            self._chk(lib().fhh_final_shares(self._h, ctypes.byref(nf), ctypes.byref(lv), ptr(paths),
                                             ptr(vals, u32p)))
        bits = paths[:, :, :L].astype(bool).tolist()
        return [Result(bits[k], limbs10_to_int(vals[k])) for k in range(F)]

    def export_states(self):
        """EvalStates of the frontier (or pending children) as [node][n][d][2] seed/t/y."""
        nn = ctypes.c_uint64()
        self._chk(lib().fhh_export_states(self._h, ctypes.byref(nn), None, None, None))
        F, n, d = int(nn.value), self.num_clients(), self.n_dims
        seeds = np.zeros((F, n, d, 2, 16), np.uint8)
        t = np.zeros((F, n, d, 2), np.uint8)
        y = np.zeros((F, n, d, 2), np.uint8)
        self._chk(lib().fhh_export_states(self._h, ctypes.byref(nn), ptr(seeds), ptr(t), ptr(y)))
        return seeds, t, y

    def stats(self) -> dict:
        s = FhhStats()
        self._chk(lib().fhh_get_stats(self._h, ctypes.byref(s)))
        return {k: getattr(s, k) for k, _ in FhhStats._fields_}

    def set_timing(self, every: int):
        """0: no k_expand events; 1: time every launch; K > 1: every K-th level-loop launch."""
        self._chk(lib().fhh_set_timing(self._h, every))

    def set_variant(self, variant: int):
        """Select the k_expand variant (bit-identical outputs, different speed)."""
        self._chk(lib().fhh_set_variant(self._h, variant))

    def set_expand_grid(self, blocks: int):
        """Tests / diagnostics: run k_expand on `blocks` workgroups (1 .. the variant's own grid)
        instead of the occupancy-derived grid. `set_variant` drops the override: call it first."""
        self._chk(lib().fhh_set_expand_grid(self._h, blocks))

    def set_protocol_grid(self, blocks: int):
        """Test / diagnostic: cap the grid of every GC / OT launch that sizes itself from the CU count at
        `blocks` workgroups (0: the device rule again). Outputs do not depend on it."""
        self._chk(lib().fhh_set_protocol_grid(self._h, blocks))

    def protocol_grid(self, family: int, need: int) -> int:
        """Test / diagnostic: the grid the launchers of `family` (FHH_GRID_*) use for `need` workgroups."""
        grid = ctypes.c_int(0)
        self._chk(lib().fhh_protocol_grid(self._h, family, need, ctypes.byref(grid)))
        return grid.value

    def set_table_row_major(self, on: bool):
        """Tests / diagnostics: the level loop and gc.table_cot run the garbled tables of b = 3, 4 bits (d = 2) on
        the row-major labels (the transpose pass + the row-major kernels) instead of the default tile-major
        kernels. Same outputs."""
        self._chk(lib().fhh_set_table_row_major(self._h, 1 if on else 0))

    def reset_stats(self):
        self._chk(lib().fhh_reset_stats(self._h))

    def reset(self):
        self._chk(lib().fhh_reset(self._h))

    def party_set_server(self, server: int):
        """Which server of the pair this collection is (0, 1; -1: unset, the default), until `reset`: with it
        set, fhh_party_node_sums negates the sums of the children this server ran in the other server's usual
        role, so that v0 - v1 is the count whoever garbled a child (a level split between the servers)."""
        self._chk(lib().fhh_party_set_server(self._h, server))

    @staticmethod
    def party_role_plan(n_children: int, chunk_children: int, level: int, mode: int):
        """[(begin, count, garbler)] of a level's windows (fhh_party_role_plan; mode 0 fixed, 1 swapped, 2 by
        level, 3 split): the counts are the real ones, also for a one-window level."""
        nw = ctypes.c_uint64(0)
        check(lib().fhh_party_role_plan(n_children, chunk_children, level, mode, 0, ctypes.byref(nw), None, None, None))
        W = nw.value
        begin, count, garbler = np.zeros(W, np.uint64), np.zeros(W, np.uint64), np.zeros(W, np.uint8)
        check(lib().fhh_party_role_plan(n_children, chunk_children, level, mode, W, ctypes.byref(nw), ptr(begin, u64p),
                                        ptr(count, u64p), ptr(garbler)))
        return [(int(b), int(c), int(g)) for b, c, g in zip(begin, count, garbler)]

    # ---- leader-side static helpers (collect.rs:945-1029) ------------------------------------
    @staticmethod
    def keep_values(nclients: int, threshold: int, vals0, vals1):
        v0 = np.ascontiguousarray(np.asarray(vals0, np.uint64))
        v1 = np.ascontiguousarray(np.asarray(vals1, np.uint64))
        if v0.shape != v1.shape:
            raise FhhError("keep_values: vals0.len() != vals1.len() (collect.rs:946)")
        keep = np.zeros(v0.size, np.uint8)
        check(lib().fhh_keep_values(threshold, ptr(v0, u64p), ptr(v1, u64p), v0.size, ptr(keep)))
        return keep.astype(bool)

    @staticmethod
    def keep_values_ring32(nclients: int, threshold: int, vals0, vals1):
        """keep_values on the servers' Z_2^32 sums (two_party_crawl form "table32"): keep iff
        (v0 - v1) mod 2^32 >= threshold. The client total must be below 2^32 (the count is then the same
        integer as in FE); a threshold or value of 2^32 or more is refused (FE sums fed in by mistake)."""
        if nclients >= 1 << 32:
            raise FhhError("keep_values_ring32: the client total must be below 2^32")
        v0 = np.ascontiguousarray(np.asarray(vals0, np.uint64))
        v1 = np.ascontiguousarray(np.asarray(vals1, np.uint64))
        if v0.shape != v1.shape:
            raise FhhError("keep_values_ring32: vals0.len() != vals1.len()")
        keep = np.zeros(v0.size, np.uint8)
        check(lib().fhh_keep_values_ring32(threshold, ptr(v0, u64p), ptr(v1, u64p), v0.size, ptr(keep)))
        return keep.astype(bool)

    @staticmethod
    def keep_values_last(nclients: int, threshold: int, vals0, vals1):
        if len(vals0) != len(vals1):
            raise FhhError("keep_values_last: vals0.len() != vals1.len() (collect.rs:967)")
        a = np.array([int_to_limbs(v, 10) for v in vals0], np.uint32).reshape(-1, 10)
        b = np.array([int_to_limbs(v, 10) for v in vals1], np.uint32).reshape(-1, 10)
        keep = np.zeros(len(vals0), np.uint8)
        check(lib().fhh_keep_values_last(threshold, ptr(a, u32p), ptr(b, u32p), len(vals0), ptr(keep)))
        return keep.astype(bool)

    @staticmethod
    def final_values(res0, res1):
        if len(res0) != len(res1):
            raise FhhError("final_values: res0.len() != res1.len() (collect.rs:1008)")
        for r0, r1 in zip(res0, res1):
            if r0.path != r1.path:
                raise FhhError("final_values: paths differ (collect.rs:1012)")
        a = np.array([int_to_limbs(r.value, 10) for r in res0], np.uint32).reshape(-1, 10)
        b = np.array([int_to_limbs(r.value, 10) for r in res1], np.uint32).reshape(-1, 10)
        out = np.zeros((len(res0), 8), np.uint32)
        check(lib().fhh_final_values(ptr(a, u32p), ptr(b, u32p), len(res0), ptr(out, u32p)))
        return [Result(r.path, limbs10_to_int(out[k])) for k, r in enumerate(res0)]


def gen_keys_pair(c0: KeyCollection, c1: KeyCollection, left_bits: np.ndarray, right_bits: np.ndarray,
                  root_seeds: np.ndarray):
    """Leader-side batched interval keygen on the GPU (ibDCF.rs:84-188), server 0's keys into
    c0 and server 1's into c1."""
    n, d, L = left_bits.shape
    if right_bits.shape != (n, d, L) or root_seeds.shape != (n, d, 2, 2, 16):
        raise FhhError("gen_keys_pair: shape mismatch")
    lb = np.ascontiguousarray(left_bits, np.uint8)
    rb = np.ascontiguousarray(right_bits, np.uint8)
    rs = np.ascontiguousarray(root_seeds, np.uint8)
    check(lib().fhh_gen_keys_pair(c0.handle, c1.handle, n, ptr(lb), ptr(rb), ptr(rs)), c0.handle)


def _ball_src(points: np.ndarray, ball: int, form: str, n_dims: int, data_len: int, root_seeds, seed, seed_first: int):
    """(fhh_ball_src, n, the arrays it points into) of points in the form's layout: "bits" uint8
    [n][d][ceil(L / 8)] (`workload.pack_points`), "coords" int16 [n][2] (lat, long)."""
    if form not in ("bits", "coords"):
        raise FhhError(f"ball source: unknown form {form!r} (bits, coords)")
    if form == "bits":
        pts = np.ascontiguousarray(points, np.uint8)
        want = (n_dims, (data_len + 7) // 8)
    else:
        pts = np.ascontiguousarray(points, np.int16)
        want = (2,)
    if pts.ndim != len(want) + 1 or pts.shape[1:] != want:
        raise FhhError(f"ball source: points of shape {pts.shape}, expected [n]{list(want)} for form {form!r}")
    n = pts.shape[0]
    src = FhhBallSrc()
    src.form = FHH_BALL_BITS if form == "bits" else FHH_BALL_COORDS
    src.ball = int(ball)
    src.points = pts.ctypes.data
    rs = None
    if root_seeds is not None:
        rs = np.ascontiguousarray(root_seeds, np.uint8)
        if rs.shape != (n, n_dims, 2, 2, 16):
            raise FhhError("ball source: root_seeds must be [n][d][2][2][16]")
        src.root_seeds = ptr(rs)
    else:
        if seed is None or len(bytes(seed)) != 32:
            raise FhhError("ball source: a 32-byte seed is needed when no root_seeds are given")
        src.seed[:] = bytes(seed)
    src.seed_first = int(seed_first)
    return src, n, (pts, rs)


def ball_bounds(points: np.ndarray, ball: int, *, n_dims: int, data_len: int, form: str = "bits", root_seeds=None,
                seed=None, seed_first: int = 0):
    """fhh_ball_bounds (host arithmetic, no GPU): (left_bits, right_bits [n][d][L], root_seeds [n][d][2][2][16]) —
    what `gen_keys_pair` needs to make the keys `gen_keys_ball` makes from the same arguments. Raises on a carry
    out (the reference panics, ibDCF.rs:182), naming the lowest (client, dim)."""
    src, n, keep = _ball_src(points, ball, form, n_dims, data_len, root_seeds, seed, seed_first)
    left = np.zeros((n, n_dims, data_len), np.uint8)
    right = np.zeros((n, n_dims, data_len), np.uint8)
    roots = np.zeros((n, n_dims, 2, 2, 16), np.uint8)
    bad = ctypes.c_uint64()
    check(lib().fhh_ball_bounds(n_dims, data_len, n, ctypes.byref(src), ptr(left), ptr(right), ptr(roots),
                                ctypes.byref(bad)))
    del keep
    return left, right, roots


def gen_keys_ball(c0: KeyCollection, c1: KeyCollection, points: np.ndarray, ball: int, form: str = "bits",
                  root_seeds=None, seed=None, seed_first: int = 0):
    """The leader's `gen_l_inf_ball` (form "bits", ibDCF.rs:175-188) / `gen_l_inf_ball_from_coords` ("coords",
    ibDCF.rs:189-205) for a population, on the GPU: server 0's keys into c0 and server 1's into c1 (both empty).
    The bounds are computed in the keygen kernel from the packed points; the root seeds are `root_seeds` or, from
    a 32-byte `seed`, the ChaCha20 block of (seed_first + client, dim): the same keys however the population is
    cut into calls. A (seed, client index) pair must not be used twice."""
    src, n, keep = _ball_src(points, ball, form, c0.n_dims, c0.depth, root_seeds, seed, seed_first)
    check(lib().fhh_gen_keys_ball(c0.handle, c1.handle, n, ctypes.byref(src)), c0.handle)
    del keep


def audit_plan(n_dims: int, data_len: int, n: int, grid_blocks: int) -> dict:
    """fhh_audit_plan (host arithmetic, no GPU): the audit kernel's launch for n clients on at most grid_blocks
    workgroups — items, waves, trips of the grid-stride loop, last_trip_items, aes_blocks, n_checks."""
    names = ("items", "waves", "trips", "last_trip_items", "aes_blocks", "n_checks")
    v = [ctypes.c_uint64() for _ in names]
    check(lib().fhh_audit_plan(n_dims, data_len, n, grid_blocks, *[ctypes.byref(x) for x in v]))
    return {k: int(x.value) for k, x in zip(names, v)}


def audit_probes(points: np.ndarray, ball: int, *, n_dims: int, data_len: int, form: str = "bits") -> np.ndarray:
    """fhh_audit_probes (host arithmetic, no GPU): the audit's probes l - 1, l, a, r, r + 1 mod 2^L of every
    (client, dim) as uint8 [n][d][5][L], a byte per bit, MSB first. Raises on a carry out, naming the lowest
    (client, dim)."""
    src, n, keep = _ball_src(points, ball, form, n_dims, data_len, None, bytes(32), 0)
    out = np.zeros((n, n_dims, 5, data_len), np.uint8)
    bad = ctypes.c_uint64()
    check(lib().fhh_audit_probes(n_dims, data_len, n, ctypes.byref(src), ptr(out), ctypes.byref(bad)))
    del keep
    return out


def leader_requests_plan(n_dims: int, data_len: int, n: int):
    """fhh_leader_requests_plan (host arithmetic, no GPU): (items, waves, trips) of the fused leader kernel's launch
    for n clients — the work items, the waves the launch gets, the trips of its grid-stride loop."""
    items, waves, trips = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    check(lib().fhh_leader_requests_plan(n_dims, data_len, n, ctypes.byref(items), ctypes.byref(waves),
                                         ctypes.byref(trips)))
    return items.value, waves.value, trips.value


def leader_requests_ball(c: KeyCollection, points: np.ndarray, ball: int, form: str = "bits", root_seeds=None,
                         seed=None, seed_first: int = 0, batch: int = 0, device_output: bool = False, out=None):
    """The leader's whole step in one call (leader.rs:130-163, 391-415): the points' keys made and serialized by
    one kernel into both servers' `add_keys` requests of `batch` clients (0: one request), with no key storage:
    `c` gives the device and the shape and is otherwise unchanged (it may be empty, or in the middle of a crawl).
    The bytes are those of `gen_keys_ball` + `export_keys_bincode(0, n, batch)` on each server's collection.
    Returns two uint8 arrays (server 0, server 1), each the requests back to back — into `out` = (out0, out1),
    uint8 arrays of at least that size, where given. With device_output: (ptr0, ptr1, nbytes), the addresses of
    the two request buffers in `c`'s device memory as integers, as the party ABI hands out its device messages;
    they are valid until the next such call on `c`, its reset or close."""
    src, n, keep = _ball_src(points, ball, form, c.n_dims, c.depth, root_seeds, seed, seed_first)
    if device_output:
        p0, p1, nbytes = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64()
        check(lib().fhh_leader_requests_ball_device(c.handle, n, ctypes.byref(src), batch, ctypes.byref(p0),
                                                    ctypes.byref(p1), ctypes.byref(nbytes)), c.handle)
        del keep
        return p0.value, p1.value, nbytes.value
    got = ctypes.c_uint64()
    if out is None:
        need = ctypes.c_uint64()
        if n:   # n = 0 is the library's to refuse
            check(lib().fhh_bincode_request_bytes(c.n_dims, c.depth, n, batch, ctypes.byref(need)))
        out = np.empty(need.value, np.uint8), np.empty(need.value, np.uint8)
    out0, out1 = out
    if out0.dtype != np.uint8 or out1.dtype != np.uint8 or out0.ndim != 1 or out1.ndim != 1:
        raise FhhError("leader_requests_ball: out must be two one-dimensional uint8 arrays")
    check(lib().fhh_leader_requests_ball(c.handle, n, ctypes.byref(src), batch, ptr(out0), ptr(out1),
                                         min(out0.size, out1.size), ctypes.byref(got)), c.handle)
    del keep
    return out0[:got.value], out1[:got.value]


def sim_eq_count(c0: KeyCollection, c1: KeyCollection, C: int) -> np.ndarray:
    out = np.zeros(C, np.uint64)
    check(lib().fhh_sim_eq_count(c0.handle, c1.handle, ptr(out, u64p)), c0.handle)
    return out


def sim_ot_sums(c0: KeyCollection, c1: KeyCollection, C: int, prf_seed: int, last: bool):
    if last:
        a = np.zeros((C, 10), np.uint32)
        b = np.zeros((C, 10), np.uint32)
        check(lib().fhh_sim_ot_sums(c0.handle, c1.handle, prf_seed, a.ctypes.data, b.ctypes.data), c0.handle)
        return [limbs10_to_int(r) for r in a], [limbs10_to_int(r) for r in b]
    a = np.zeros(C, np.uint64)
    b = np.zeros(C, np.uint64)
    check(lib().fhh_sim_ot_sums(c0.handle, c1.handle, prf_seed, a.ctypes.data, b.ctypes.data), c0.handle)
    return [int(x) for x in a], [int(x) for x in b]


__all__ = ["KeyCollection", "Result", "gen_keys_pair", "gen_keys_ball", "ball_bounds", "leader_requests_ball",
           "leader_requests_plan", "sim_eq_count", "sim_ot_sums", "FE_P", "FE255_P"]
