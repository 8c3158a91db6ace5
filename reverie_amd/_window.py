"""What `DeviceCompactor`, `DevicePruner` and `DeviceFolder` share: the handle of a windowed stage (rv_compactor, rv_pruner,
rv_folder) on a context, the form its feeds take, and the Input counts of a piece."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .ops import OP_DTYPE, program
from .proof import _device_ops, _is_device_ops, _ptr


def info_dict(ci) -> dict:
    return {n: int(getattr(ci, n)) for n, _ in ci._fields_}


def input_counts(ops):
    """the (GF(2), Z64) Input ops of a piece: a host array, or a torch GPU tensor of packed rv_op records"""
    if not _is_device_ops(ops):  # (counted where the records still are a host array)
        a = program(ops)
        inputs = a["opcode"] == 0
        return int(np.count_nonzero(inputs & (a["domain"] == 0))), int(np.count_nonzero(inputs & (a["domain"] == 1)))
    recs = ops.reshape(-1, OP_DTYPE.itemsize)  # (domain and opcode are a record's first two bytes)
    inputs = recs[:, 1] == 0
    return int((inputs & (recs[:, 0] == 0)).sum()), int((inputs & (recs[:, 0] == 1)).sum())


class _DeviceStage:
    """a windowed stage's handle on its context.  The subclass begins the stage into `self.handle` and names itself:"""

    _what = ""  # the class, as the messages name it
    _destroy = ""  # rv_*_destroy
    _info_of = (None, "")  # the rv_*_info struct of _lib and its getter

    def __init__(self, ctx):
        self.ctx = ctx
        self.handle = C.c_void_p()
        self.info = None

    def _ops(self, ops):
        """-> (pointer, n_ops, on device, what keeps the memory alive)"""
        if _is_device_ops(ops):
            d_ops, n_ops, _ = _device_ops(ops, self.ctx, self._what)
            return C.c_void_p(d_ops), n_ops, 1, ops
        a = program(ops) if len(ops) else np.zeros(0, OP_DTYPE)
        return _ptr(a), len(a), 0, a

    def get_info(self) -> dict:
        struct, getter = self._info_of
        ci = struct()
        _lib.check(getattr(_lib.lib(), getter)(self.handle, C.byref(ci)))
        return info_dict(ci)

    def close(self) -> None:
        """gives the stage's device memory back to its context (a context that was closed first took its memory with it: the handle
        is dropped then, not destroyed)"""
        if self.handle:
            if self.ctx.handle:
                getattr(_lib.lib(), self._destroy)(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        import sys

        if sys.is_finalizing():  # (finalisers run in no order then: the context and the runtime may be gone; the process ends anyway)
            return
        try:
            self.close()
        except Exception:
            pass
