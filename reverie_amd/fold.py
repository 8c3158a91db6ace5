"""Constants folded in op lists (include/reverie_amd.h: rv_ops_fold / rv_ops_fold_device).

Real statements wire public values into blocks written for secret ones: the IV and the padding block of a SHA-256, the round keys of
a cipher with a public key, a comparison against a public bound.  `fold_ops` rewrites record for record: a gate whose operands are
all known becomes a Const, a Mul with one known operand a MulConst (or a Const 0), an Add or Sub with one known operand an AddConst
or SubConst.  Nothing is dropped, moved or renumbered, and every wire's value stays what it was; `prune_ops` afterwards drops the
Consts nothing reads any more.  The order is fold, then prune, then `compact_wires`.

THE PROOF OF A FOLDED LIST IS THE PROOF OF THAT LIST, not of the original: a folded Mul or B2A no longer contributes to it.  Prover
and verifier both fold, or the folded program is the file that is shipped."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _lib
from .ops import OP_DTYPE, largest_wires, program
from .proof import Context, _device_ops, _is_device_ops, _ptr


def _info(fi) -> dict:
    return {n: int(getattr(fi, n)) for n, _ in fi._fields_}


def fold_ops(ops, wire_counts: Optional[Tuple[int, int]] = None, ctx: Optional[Context] = None, inplace: bool = False, count_only: bool = False):
    """-> (ops, info): the folded records (as many as went in) and rv_fold_info as a dict.

    Host ops (an OP_DTYPE array or anything `program` takes) go through the forward sweep and need no GPU; wire_counts None means
    `largest_wires(ops)`.  A torch GPU tensor of packed rv_op records (the layouts of `Circuit.from_device_ops`) is folded by kernels
    on the context's GPU: the records come back as a new uint8 tensor [n, 24] on the same device; wire_counts must be given then.
    inplace: the records are written into the argument (an OP_DTYPE array or a GPU tensor), which is returned.  count_only: nothing
    is written -- (None, info).  An op list the compiler would refuse raises the compiler's error."""
    fi = _lib.FoldInfo()
    L = _lib.lib()
    if _is_device_ops(ops):
        if wire_counts is None:
            raise ValueError("fold_ops of a device op list needs wire_counts")
        d_ops, n_ops, ctx = _device_ops(ops, ctx, "fold_ops")
        import torch

        head = (ctx.handle, C.c_void_p(d_ops) if n_ops else None, C.c_size_t(n_ops), C.c_size_t(int(wire_counts[0])), C.c_size_t(int(wire_counts[1])))
        if count_only:
            _lib.check(L.rv_ops_fold_device(*head, None, C.byref(fi)))
            return None, _info(fi)
        out = ops if inplace else torch.empty((n_ops, OP_DTYPE.itemsize), dtype=torch.uint8, device=ops.device)
        _lib.check(L.rv_ops_fold_device(*head, C.c_void_p(d_ops if inplace else out.data_ptr()) if n_ops else None, C.byref(fi)))
        return out, _info(fi)
    if inplace:
        if not (isinstance(ops, np.ndarray) and ops.dtype == OP_DTYPE and ops.flags.c_contiguous and ops.flags.writeable):
            raise ValueError("fold_ops(inplace=True) needs a writable contiguous OP_DTYPE array or a GPU tensor")
    else:
        ops = program(ops) if len(ops) else np.zeros(0, OP_DTYPE)
    if wire_counts is None:
        wire_counts = largest_wires(ops) if len(ops) else (0, 0)
    head = (_ptr(ops), C.c_size_t(len(ops)), C.c_size_t(int(wire_counts[0])), C.c_size_t(int(wire_counts[1])))
    if count_only:
        _lib.check(L.rv_ops_fold(*head, None, C.byref(fi)))
        return None, _info(fi)
    out = ops if inplace else np.empty_like(ops)
    _lib.check(L.rv_ops_fold(*head, _ptr(out), C.byref(fi)))
    return out, _info(fi)
