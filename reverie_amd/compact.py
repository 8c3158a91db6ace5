"""Wire indices compacted by liveness (include/reverie_amd.h: rv_ops_compact_wires / rv_ops_compact_wires_device / rv_compactor_*;
DESIGN §17).

A stream's wire store has one row per wire index, so an op list in SSA form (a Bristol file, a list a parallel generator wrote) needs
a row per gate.  `compact_wires` renumbers the wires of a whole list so that an index is reused after its value's last reader.  The
proof of the new list under the new counts is byte for byte the proof of the old one; wire values (`KEEP_WIRES`, `evaluate*`) refer to
the new indices -- the renumbered `dst` of an op is where its value lives.

`DeviceCompactor` and `compact_pieces` give the same result for a list that is read in windows (a program file, a Bristol text): the
list passes through twice (three times when it holds a B2A op), and device memory follows the window and the OLD wire counts, not the
list's length."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _lib
from ._window import _DeviceStage, info_dict as _info, input_counts
from .ops import OP_DTYPE, largest_wires, program
from .proof import Context, _device_ops, _is_device_ops, _ptr


def compact_wires(ops, wire_counts: Optional[Tuple[int, int]] = None, ctx: Optional[Context] = None):
    """-> (ops, (z64_wires, gf2_wires), info): the list renumbered, the new wire counts and rv_compact_info as a dict.

    Host ops (an OP_DTYPE array or anything `program` takes) go through the sequential sweep and need no GPU; wire_counts None means
    `largest_wires(ops)`.  A torch GPU tensor of packed rv_op records (the layouts of `Circuit.from_device_ops`) is compacted where it
    lies by kernels on the context's GPU and comes back as a new tensor of the same shape, dtype and device; wire_counts must be given
    then.  The input is left as it is either way.  An op list the compiler would refuse raises the compiler's error."""
    ci = _lib.CompactInfo()
    if _is_device_ops(ops):
        if wire_counts is None:
            raise ValueError("compact_wires of a device op list needs wire_counts")
        d_ops, n_ops, ctx = _device_ops(ops, ctx, "compact_wires")
        import torch

        out = torch.empty_like(ops)
        _lib.check(_lib.lib().rv_ops_compact_wires_device(ctx.handle, C.c_void_p(d_ops), C.c_size_t(n_ops), C.c_size_t(int(wire_counts[0])),
                                                          C.c_size_t(int(wire_counts[1])), C.c_void_p(out.data_ptr()), C.byref(ci)))
    else:
        ops = program(ops) if len(ops) else np.zeros(0, OP_DTYPE)
        if wire_counts is None:
            wire_counts = largest_wires(ops)
        out = np.empty_like(ops)
        _lib.check(_lib.lib().rv_ops_compact_wires(_ptr(ops), C.c_size_t(len(ops)), C.c_size_t(int(wire_counts[0])), C.c_size_t(int(wire_counts[1])),
                                                   _ptr(out), C.byref(ci)))
    info = _info(ci)
    return out, (info["z64_wires"], info["gf2_wires"]), info


class DeviceCompactor(_DeviceStage):
    """rv_compactor: `compact_wires` for an op list that arrives in feeds.  scan(ops)... scan_end() (again, when it says so), then
    feed(ops)... -> the renumbered records, feed by feed; rewind() starts the rewrite pass again.  The two passes may be cut
    differently.  ops: an OP_DTYPE array (uploaded) or a torch GPU tensor of packed rv_op records."""

    _what, _destroy, _info_of = "DeviceCompactor", "rv_compactor_destroy", (_lib.CompactorInfo, "rv_compactor_get_info")

    def __init__(self, wire_counts: Tuple[int, int], ctx: Optional[Context] = None):
        super().__init__(ctx or Context.default())
        self.wire_counts = None
        _lib.check(_lib.lib().rv_compactor_begin(self.ctx.handle, C.c_size_t(int(wire_counts[0])), C.c_size_t(int(wire_counts[1])),
                                                 C.byref(self.handle)))

    def scan(self, ops) -> None:
        p, n, dev, _keep = self._ops(ops)
        _lib.check(_lib.lib().rv_compactor_scan(self.handle, p, C.c_size_t(n), C.c_int(dev)))

    def scan_end(self) -> bool:
        """-> again: True when the list holds a B2A op and has to be scanned once more"""
        again, ci = C.c_int(0), _lib.CompactInfo()
        _lib.check(_lib.lib().rv_compactor_scan_end(self.handle, C.byref(again), C.byref(ci)))
        if not again.value:
            self.info = _info(ci)
            self.wire_counts = (self.info["z64_wires"], self.info["gf2_wires"])
        return bool(again.value)

    def feed(self, ops, out=None):
        """-> the feed's renumbered records as a new uint8 GPU tensor [n, 24] (or `out`, a GPU tensor that may be a device `ops`)"""
        import torch

        p, n, dev, _keep = self._ops(ops)
        if out is None:
            out = torch.empty((n, OP_DTYPE.itemsize), dtype=torch.uint8, device=f"cuda:{self.ctx.device}")
        _lib.check(_lib.lib().rv_compactor_feed(self.handle, p, C.c_size_t(n), C.c_int(dev), C.c_void_p(out.data_ptr()) if n else None))
        return out

    def rewind(self) -> None:
        _lib.check(_lib.lib().rv_compactor_rewind(self.handle))

    def get_info(self) -> dict:
        """rv_compactor_info: total_ops, state_bytes, peak_feed_bytes, scans, b2a"""
        return super().get_info()


def compact_pieces(pieces, wire_counts: Tuple[int, int], ctx: Optional[Context] = None):
    """-> (new wire counts, pieces2, info) for `pieces` as `stream.prove_streaming_pieces` takes them: a callable that returns a fresh
    iterator of (ops, Input counts).  The scan pass runs here (twice for a list with B2A ops).  `pieces2` is such a callable too: every
    call reads the source again and yields (the piece's renumbered records as a GPU tensor, the source's Input counts) -- records map
    1:1, so the counts pass through; a pass has to be read to its end before the next one begins (rv_compactor_rewind refuses a short
    pass).  info: rv_compact_info as a dict, with "compactor" (rv_compactor_info) beside it; the
    compactor lives as long as `pieces2`."""
    if not callable(pieces):
        raise TypeError("compact_pieces reads the pieces several times: pass a callable that returns a fresh iterator")
    dc = DeviceCompactor(wire_counts, ctx)
    again = True
    while again:
        for ops, _ in pieces():
            if ops is not None and len(ops):
                dc.scan(ops)
        again = dc.scan_end()
    started = [False]

    def pieces2():
        if started[0]:
            dc.rewind()
        started[0] = True
        for ops, counts in pieces():
            if ops is None or len(ops) == 0:
                continue
            if counts is None and not _is_device_ops(ops):  # (a device piece's counts stay None: the stream counts them where it needs them)
                counts = input_counts(ops)
            yield dc.feed(ops), counts

    pieces2.compactor = dc
    info = dict(dc.info)
    info["compactor"] = dc.get_info()
    return dc.wire_counts, pieces2, info
