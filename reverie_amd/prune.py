"""Ops no assertion or output depends on, dropped (include/reverie_amd.h: rv_ops_prune / rv_ops_prune_device).

A statement uses part of what its function blocks compute, and the linker emits every record of every instance.  A dead Mul is a
correction and a broadcast per repetition in the proof, a dead B2A 442 GF(2) steps, a dead Random a mask.  `prune_ops` keeps the
roots -- every AssertZero, Input and SizeHint, and the values the caller's output indices end on -- and what they depend on, and
drops the rest; the kept records stay as they are, in order, so nothing is renumbered and the wire counts stay valid.

THE PROOF OF A PRUNED LIST IS THE PROOF OF THAT LIST, not of the original: unlike `compact_wires` this changes proof bytes (that is
its purpose).  Prover and verifier both prune, with the same outputs, or the pruned program is the file that is shipped.  Final wire
values change too (`keep_wires`, `evaluate*`): a dropped op's destination keeps whatever was there before."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._window import _DeviceStage, info_dict as _info, input_counts
from .ops import OP_DTYPE, largest_wires, program
from .proof import Context, _device_ops, _is_device_ops, _ptr


def _outputs(outputs) -> np.ndarray:
    a = np.asarray(list(outputs) if not isinstance(outputs, np.ndarray) else outputs, dtype=np.int64).reshape(-1)
    if a.size and (a.min() < 0 or a.max() > 0xFFFFFFFF):
        raise ValueError("an output index is a wire index: 0 .. 2^32 - 1")
    return np.ascontiguousarray(a.astype(np.uint32))


def prune_ops(ops, wire_counts: Optional[Tuple[int, int]] = None, outputs_gf2: Sequence[int] = (), outputs_z64: Sequence[int] = (),
              ctx: Optional[Context] = None, count_only: bool = False):
    """-> (ops, info, old_index): the kept records, rv_prune_info as a dict, and for every kept record its index in the old list.

    Host ops (an OP_DTYPE array or anything `program` takes) go through the backward sweep and need no GPU; wire_counts None means
    `largest_wires(ops)`.  A torch GPU tensor of packed rv_op records (the layouts of `Circuit.from_device_ops`) is pruned by kernels
    on the context's GPU: the records come back as a new uint8 tensor [n_kept, 24] and old_index as an int32 tensor [n_kept] on the
    same device (the bits are uint32; op counts stay below 2^31); wire_counts must be given then.  The input is left as it is.
    count_only: nothing is written -- (None, info, None), the "what would it save" call.  An op list the compiler would refuse raises
    the compiler's error; an output index at or above its domain's final wire count raises ReverieError (ARG)."""
    pi, n_out = _lib.PruneInfo(), C.c_size_t(0)
    og, oz = _outputs(outputs_gf2), _outputs(outputs_z64)
    L = _lib.lib()
    if _is_device_ops(ops):
        if wire_counts is None:
            raise ValueError("prune_ops of a device op list needs wire_counts")
        d_ops, n_ops, ctx = _device_ops(ops, ctx, "prune_ops")
        import torch

        head = (C.c_void_p(d_ops) if n_ops else None, C.c_size_t(n_ops), C.c_size_t(int(wire_counts[0])), C.c_size_t(int(wire_counts[1])),
                _ptr(og), C.c_size_t(og.size), _ptr(oz), C.c_size_t(oz.size))
        if count_only:
            _lib.check(L.rv_ops_prune_device(ctx.handle, *head, None, C.c_size_t(0), C.byref(n_out), None, C.byref(pi)))
            return None, _info(pi), None
        # one call, with room for everything; a result of less than half the list is copied out of that room
        out = torch.empty((n_ops, OP_DTYPE.itemsize), dtype=torch.uint8, device=ops.device)
        old = torch.empty((n_ops,), dtype=torch.int32, device=ops.device)
        _lib.check(L.rv_ops_prune_device(ctx.handle, *head, C.c_void_p(out.data_ptr()) if n_ops else None, C.c_size_t(n_ops), C.byref(n_out),
                                         C.c_void_p(old.data_ptr()) if n_ops else None, C.byref(pi)))
        kept = int(n_out.value)
        out, old = out[:kept], old[:kept]
        if 2 * kept < n_ops:
            out, old = out.clone(), old.clone()
        return out, _info(pi), old
    ops = program(ops) if len(ops) else np.zeros(0, OP_DTYPE)
    if wire_counts is None:
        wire_counts = largest_wires(ops) if len(ops) else (0, 0)
    head = (_ptr(ops), C.c_size_t(len(ops)), C.c_size_t(int(wire_counts[0])), C.c_size_t(int(wire_counts[1])), _ptr(og), C.c_size_t(og.size),
            _ptr(oz), C.c_size_t(oz.size))
    if count_only:
        _lib.check(L.rv_ops_prune(*head, None, C.c_size_t(0), C.byref(n_out), None, C.byref(pi)))
        return None, _info(pi), None
    out, old = np.empty_like(ops), np.empty(len(ops), np.uint32)
    _lib.check(L.rv_ops_prune(*head, _ptr(out), C.c_size_t(len(out)), C.byref(n_out), _ptr(old), C.byref(pi)))
    kept = int(n_out.value)
    return out[:kept].copy(), _info(pi), old[:kept].copy()


# ---- the same for a list that passes through in windows (rv_pruner_*) ----
class DevicePruner(_DeviceStage):
    """rv_pruner: `prune_ops` for an op list that arrives in feeds.  scan(ops)... scan_end(); mark(ops)... with the windows from the
    LAST to the first (each window's ops in list order), mark_end() -> rv_prune_info; then feed(ops)... forwards -> the kept records,
    feed by feed; rewind() starts the emit pass again.  The three passes may be cut differently.  ops: an OP_DTYPE array (uploaded)
    or a torch GPU tensor of packed rv_op records.  wire_counts: (z64, gf2) as stated; the outputs as in `prune_ops`."""

    _what, _destroy, _info_of = "DevicePruner", "rv_pruner_destroy", (_lib.PrunerInfo, "rv_pruner_get_info")

    def __init__(self, wire_counts: Tuple[int, int], outputs_gf2: Sequence[int] = (), outputs_z64: Sequence[int] = (), ctx: Optional[Context] = None):
        super().__init__(ctx or Context.default())
        og, oz = _outputs(outputs_gf2), _outputs(outputs_z64)
        _lib.check(_lib.lib().rv_pruner_begin(self.ctx.handle, C.c_size_t(int(wire_counts[0])), C.c_size_t(int(wire_counts[1])), _ptr(og),
                                              C.c_size_t(og.size), _ptr(oz), C.c_size_t(oz.size), C.byref(self.handle)))

    def scan(self, ops) -> None:
        p, n, dev, _keep = self._ops(ops)
        _lib.check(_lib.lib().rv_pruner_scan(self.handle, p, C.c_size_t(n), C.c_int(dev)))

    def scan_end(self) -> None:
        _lib.check(_lib.lib().rv_pruner_scan_end(self.handle))

    def mark(self, ops) -> int:
        """-> the ops of the feed that are kept"""
        p, n, dev, _keep = self._ops(ops)
        kept = C.c_size_t(0)
        _lib.check(_lib.lib().rv_pruner_mark(self.handle, p, C.c_size_t(n), C.c_int(dev), C.byref(kept)))
        return int(kept.value)

    def mark_end(self) -> dict:
        """-> rv_prune_info as a dict (also .info)"""
        pi = _lib.PruneInfo()
        _lib.check(_lib.lib().rv_pruner_mark_end(self.handle, C.byref(pi)))
        self.info = _info(pi)
        return self.info

    def feed(self, ops):
        """-> (the feed's kept records as a uint8 GPU tensor [n_out, 24], their indices in the whole old list as an int32 GPU tensor
        [n_out]; the bits are uint32)"""
        import torch

        p, n, dev, _keep = self._ops(ops)
        device = f"cuda:{self.ctx.device}"
        out = torch.empty((n, OP_DTYPE.itemsize), dtype=torch.uint8, device=device)
        old = torch.empty((n,), dtype=torch.int32, device=device)
        n_out = C.c_size_t(0)
        _lib.check(_lib.lib().rv_pruner_feed(self.handle, p, C.c_size_t(n), C.c_int(dev), C.c_void_p(out.data_ptr()) if n else None, C.c_size_t(n),
                                             C.byref(n_out), C.c_void_p(old.data_ptr()) if n else None))
        kept = int(n_out.value)
        out, old = out[:kept], old[:kept]
        if 2 * kept < n:
            out, old = out.clone(), old.clone()
        return out, old

    def rewind(self) -> None:
        _lib.check(_lib.lib().rv_pruner_rewind(self.handle))

    def get_info(self) -> dict:
        """rv_pruner_info: total_ops, n_kept, state_bytes, peak_feed_bytes, mark_feeds, host_feeds"""
        return super().get_info()


def window_pieces(ops, window_ops: int):
    """-> a callable that returns a fresh iterator of (window, None) over `ops` -- an OP_DTYPE array, an `np.memmap` of one (an rvops
    file's records) or a torch GPU tensor of packed rv_op records -- in windows of window_ops records, with `.backwards`: the same
    windows from the last to the first.  The windows are views; nothing is copied here."""
    if window_ops <= 0:
        raise ValueError("window_ops must be positive")
    if _is_device_ops(ops):  # (any layout `Circuit.from_device_ops` takes: uint8 [n, 24] or [n * 24], int64 / uint64 [n, 3]; as bytes)
        import torch

        if not ops.is_contiguous():
            raise ValueError("window_pieces needs a contiguous tensor of packed rv_op records")
        recs = ops.view(torch.uint8).reshape(-1, OP_DTYPE.itemsize)
    else:
        recs = ops
    n = len(recs)

    def windows(firsts):
        for first in firsts:
            yield recs[first:first + window_ops], None

    def it():
        return windows(range(0, n, window_ops))

    def backwards():
        return windows(reversed(range(0, n, window_ops)))

    it.backwards = backwards
    return it


def prune_pieces(pieces, wire_counts: Tuple[int, int], outputs_gf2: Sequence[int] = (), outputs_z64: Sequence[int] = (), backwards=None,
                 ctx: Optional[Context] = None):
    """-> (pieces2, info) for `pieces` as `stream.prove_streaming_pieces` takes them: a callable that returns a fresh iterator of
    (ops, Input counts).  `backwards`: a callable that returns a fresh iterator over the SAME LIST in windows from the last to the
    first (its cuts need not be `pieces`'); default `pieces.backwards`.  The scan pass and the mark pass run here.  `pieces2` is such
    a callable too: every call reads the source again and yields (the piece's kept records as a GPU tensor, the source's Input
    counts) -- Inputs are roots, so the counts pass through; pieces of which nothing is kept are skipped, and a pass has to be read
    to its end before the next one begins.  The wire counts do not change.  info: rv_prune_info as a dict, with "pruner"
    (rv_pruner_info) beside it; the pruner lives as long as `pieces2` (`pieces2.pruner`)."""
    if not callable(pieces):
        raise TypeError("prune_pieces reads the pieces several times: pass a callable that returns a fresh iterator")
    if backwards is None:
        backwards = getattr(pieces, "backwards", None)
    if not callable(backwards):
        raise TypeError("prune_pieces marks from the last window to the first and needs a source that can be read backwards: "
                        "LinkPlan.pieces(window_ops), prune.window_pieces(ops, window_ops) on a host array, an rvops memory map or a GPU "
                        "tensor, or backwards=<a callable>; a Bristol text or a bincode file is read forwards only: convert it to "
                        "rvops first")
    dp = DevicePruner(wire_counts, outputs_gf2, outputs_z64, ctx)
    try:
        for ops, _ in pieces():
            if ops is not None and len(ops):
                dp.scan(ops)
        dp.scan_end()
        for ops, _ in backwards():
            if ops is not None and len(ops):
                dp.mark(ops)
        info = dict(dp.mark_end())
    except BaseException:
        dp.close()
        raise
    started = [False]

    def pieces2():
        if started[0]:
            dp.rewind()
        started[0] = True
        for ops, counts in pieces():
            if ops is None or len(ops) == 0:
                continue
            if counts is None:
                counts = input_counts(ops)
            kept, _old = dp.feed(ops)
            if len(kept):
                yield kept, counts

    pieces2.pruner = dp
    info["pruner"] = dp.get_info()
    return pieces2, info
