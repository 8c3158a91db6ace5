"""Wire indices compacted by liveness (include/reverie_amd.h: rv_ops_compact_wires / rv_ops_compact_wires_device).

A stream's wire store has one row per wire index, so an op list in SSA form (a Bristol file, a list a parallel generator wrote) needs
a row per gate.  `compact_wires` renumbers the wires of a whole list so that an index is reused after its value's last reader.  The
proof of the new list under the new counts is byte for byte the proof of the old one; wire values (`KEEP_WIRES`, `evaluate*`) refer to
the new indices -- the renumbered `dst` of an op is where its value lives."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _lib
from .ops import OP_DTYPE, largest_wires, program
from .proof import Context, _device_ops, _is_device_ops, _ptr


def _info(ci) -> dict:
    return {n: int(getattr(ci, n)) for n, _ in ci._fields_}


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
