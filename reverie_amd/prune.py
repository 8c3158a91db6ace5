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
from .ops import OP_DTYPE, largest_wires, program
from .proof import Context, _device_ops, _is_device_ops, _ptr


def _info(pi) -> dict:
    return {n: int(getattr(pi, n)) for n, _ in pi._fields_}


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
