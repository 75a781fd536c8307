"""The device loop control shared by every solver engine: the 48-byte control block (``pcs::Ctrl``,
csrc/pds_ctrl.hpp) and the history buffer the finalize kernels write, their sizing and growth, and
the host's asynchronous view of the stop decision (the reference's ``while`` of
``pycsou/core/solver.py:65-66`` runs on the device; the host only learns about the stop afterwards).
"""

import ctypes

import numpy as np
import torch

from .. import _lib as L

HIST_CHUNK = 4096  # iterations of device history allocated at first; doubled as the loop goes on


def loop_buffer(numel, device, fill=None):
    """Every float64 device buffer a loop owns and lends to the kernels -- the control block, the history,
    the per-workgroup partials and the reduction workspace -- is allocated here, at exactly the size the
    C ABI advertises for it (include/pycsou_hip.h: pcs_ctrl_bytes, Ctrl.hist_len, *_nblocks, *_ws_bytes).
    `fill`: None leaves the contents as they come, else the value of every element."""
    if fill is None:
        return torch.empty(int(numel), dtype=torch.float64, device=device)
    return torch.full((int(numel),), float(fill), dtype=torch.float64, device=device)


def initial_rows(total, chunk, up_front=None):
    """History rows allocated when a loop of at most `total` iterations starts: room for the first
    chunks (a max_iter of 1e9 with accuracy_threshold doing the stopping must not allocate
    2 * max_iter doubles up front), or exactly `up_front` rows for a loop that cannot grow."""
    if up_front is not None:
        return int(up_front)
    return min(total, max(HIST_CHUNK, 2 * chunk))


def grown_rows(have, need, total):
    """Rows of a history of `have` rows once `need` rows are asked for: doubled, at most `total`."""
    if need <= have or have >= total:
        return have
    return min(total, max(2 * have, need))


class LoopControl:
    """One loop's control block and history on the device.  `hist` holds 2 doubles per row (the primal
    and dual relative improvements) + 2; `Ctrl.hist_len` is always its numel, so the finalize kernels
    stay inside it."""

    # fields of pcs::Ctrl: indices into the int32 view of `ctrl` / into its float64 view
    IT, STOPPED, MIN_ITER, MAX_ITER, HAS_DUAL, HIST_LEN = 0, 1, 2, 3, 4, 5
    THR = 4

    def __init__(self, device):
        self.lib = L.gpu()
        self.ctrl = loop_buffer(int(self.lib.pcs_ctrl_bytes()) // 8, device, 0.0)
        # a placeholder until start(): plans that hold the history pointer can be built before a loop
        self.hist = loop_buffer(2, device, float('nan'))
        self.total = 0
        self.replaced = False
        self.final = None
        self._pending, self._free = [], []

    def _fields(self):
        return self.ctrl.view(torch.int32)

    def start(self, max_iter, min_iter, thr, has_dual, chunk=1, up_front=None):
        """A fresh loop: the history sized by initial_rows (the existing buffer when it is large
        enough) and filled with NaN, the control block initialised.  Returns the most iterations the
        loop can run; `replaced` says whether `hist` is a new buffer (a captured graph or a plan keyed
        on its pointer is stale then)."""
        max_iter, min_iter = int(max_iter), int(min_iter)
        self.total = max(min_iter, max_iter) + 1
        numel = 2 * initial_rows(self.total, chunk, up_front) + 2
        self.replaced = self.hist.numel() < numel
        if self.replaced:
            self.hist = loop_buffer(numel, self.ctrl.device)
        self.hist.fill_(float('nan'))
        L.check(self.lib.pcs_ctrl_init2(L.ptr(self.ctrl), min_iter, max_iter, float(thr), int(has_dual),
                                        int(self.hist.numel()), L.stream()), 'pcs_ctrl_init2')
        self.final, self._pending = None, []
        return self.total

    def start_fixed(self, n, rows=None):
        """A loop of exactly `n` iterations that never stops early (benchmarks, the kernel timers), with
        `rows` history rows up front (default: the buffer as it is)."""
        return self.start(n, n, -1.0, 1, up_front=(self.hist.numel() - 2) // 2 if rows is None else rows)

    def reserve(self, rows):
        """Room for `rows` history rows (at most `total`): a copy twice as long with Ctrl.hist_len
        updated, both stream-ordered after every iteration already enqueued.  True when `hist` was
        replaced."""
        have = (self.hist.numel() - 2) // 2
        cap = grown_rows(have, rows, self.total)
        if cap == have:
            return False
        new = loop_buffer(2 * cap + 2, self.hist.device, float('nan'))
        new[:self.hist.numel()].copy_(self.hist)
        self._fields()[self.HIST_LEN].fill_(int(new.numel()))
        self.hist = new
        return True

    # ---- blocking reads
    def iterations(self):
        return int(self._fields()[self.IT].item())

    def stopped(self):
        return int(self._fields()[self.STOPPED].item()) != 0

    def rows(self, n):
        """The first n history rows as an (n, 2) NumPy array."""
        return self.hist[:2 * n].cpu().numpy().reshape(n, 2) if n > 0 else np.zeros((0, 2))

    # ---- the stop decision without blocking the launching thread
    def fetch(self, host):
        """Enqueue the copy of (it, stopped) into the pinned int32 pair `host`."""
        host.copy_(self._fields()[:2], non_blocking=True)

    def read_async(self):
        """fetch() into a pinned pair of the loop's own and an event behind it, for poll().  A pair is
        reused once poll() has resolved it, so at most lag + 1 are ever allocated."""
        host = self._free.pop() if self._free else torch.zeros(2, dtype=torch.int32).pin_memory()
        self.fetch(host)
        ev = torch.cuda.Event()
        ev.record()
        self._pending.append((host, ev))

    def poll(self, lag, drain=False, seen=None):
        """Resolve finished read-backs in order; returns the iteration count once the device stopped
        (None while it runs).  Blocks only to keep at most `lag` in flight (`drain`: none).
        seen(it) is called with every resolved count."""
        while self._pending and self.final is None:
            host, ev = self._pending[0]
            if not (drain or len(self._pending) > lag or ev.query()):
                break
            ev.synchronize()
            self._pending.pop(0)
            it, stopped = int(host[self.IT]), int(host[self.STOPPED])
            self._free.append(host)
            if seen is not None:
                seen(it)
            if stopped != 0:
                self.final = it
        return self.final


class LoopViews:
    """The control block and the history of the LoopControl an object holds as `ctl`."""

    ctrl = property(lambda self: self.ctl.ctrl)
    hist = property(lambda self: self.ctl.hist)


class LoopState(LoopViews):
    """What an engine whose step reduces and finalizes its own diagnostics holds of its loop on the
    device, beside the iterates: the LoopControl `ctl`, the per-workgroup norm partials and the
    workspace of the in-kernel reduce + finalize."""

    def _init_reduction(self, a, dev, nblocks_fn, ws_bytes_fn):
        """The step arguments `a` are complete but for what the loop owns: the partials of the launch's
        `nblocks_fn(a)` workgroups, the loop control, and the reduction workspace of `ws_bytes_fn(a)` bytes
        (its counters start at 0 and every launch leaves them at 0)."""
        self.nblocks = int(nblocks_fn(ctypes.byref(a)))
        self._alloc_partials(a, dev)
        self.ctl = LoopControl(dev)
        a.ctrl = self.ctrl.data_ptr()
        self.ws = loop_buffer(-(-int(ws_bytes_fn(ctypes.byref(a))) // 8), dev, 0.0)
        a.ws = self.ws.data_ptr()

    def _alloc_partials(self, a, dev):
        """[nblocks][4] doubles."""
        self.partials = loop_buffer(4 * self.nblocks, dev)
        a.partials = self.partials.data_ptr()


def worst_over_ranks(comm, values, world, device):
    """Max over ranks of each of this rank's (at most 4) timings, so that every rank takes the same
    decision from them: one all-gather of 4 doubles per rank."""
    mine = torch.tensor(list(values) + [0.0] * (4 - len(values)), dtype=torch.float64, device=device)
    allt = torch.zeros(4 * world, dtype=torch.float64, device=device)
    comm.allgather(mine, allt)
    return allt.view(world, 4).max(dim=0).values[:len(values)].tolist()


def capture_agreed(fn, comm=None, world=1, device=None):
    """fn() captured into a hipGraph, or None.  Multi-GPU: every rank must end up with a graph or none
    (captured RCCL calls pair across ranks), so the outcome is agreed collectively (min over ranks of a
    flag all-gather) and a failed capture anywhere returns None everywhere."""
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(g):
            fn()
    except Exception:  # noqa: BLE001 -- torch's capture errors and the ABI's HipError alike: every rank
        # must reach the flag all-gather below, or the others block in RCCL
        g = None
        torch.cuda.synchronize()
    if world > 1:
        flag = torch.tensor([0.0 if g is None else 1.0], dtype=torch.float64, device=device)
        allf = torch.zeros(world, dtype=torch.float64, device=device)
        comm.allgather(flag, allf)
        if not allf.min().item() > 0:
            g = None
    return g


class LaunchTimer:
    """HIP event pairs around launches on one stream: timer(name, fn) runs fn between two events,
    result() gives a statistic (ms) of each name's durations."""

    def __init__(self, stream=None):
        self.st = torch.cuda.current_stream() if stream is None else stream
        self.ev = {}

    def __call__(self, name, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(self.st)
        fn()
        e1.record(self.st)
        self.ev.setdefault(name, []).append((e0, e1))

    def result(self, stat=np.mean):
        torch.cuda.synchronize()
        return {k: float(stat([s.elapsed_time(e) for s, e in v])) for k, v in self.ev.items()}
