"""Program files of the reference CLI: bincode(`Vec<mcircuit::CombineOperation>`), read at
/root/reference/src/main.rs:66,98,122.  The (de)serialiser is C++ behind the C-ABI
(`rv_program_from_bincode` / `rv_program_to_bincode`, reverie_amd/csrc/program.cpp); this is the ctypes
wrapper.  The enum's variant order is recalled, not verifiable here — see the header.
`loads_device` / `dumps_device` are the same two on the GPU (`rv_program_from_bincode_device` / `rv_program_to_bincode_device`,
reverie_amd/csrc/bincode_dev.hip: DESIGN §19): the op list is made in, and written from, device memory."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .ops import OP_DTYPE, program


def loads(data: bytes) -> np.ndarray:
    """bincode bytes -> rv_op array"""
    data = bytes(data)
    ops = C.c_void_p()
    n = C.c_size_t()
    buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
    _lib.check(_lib.lib().rv_program_from_bincode(buf, C.c_size_t(len(data)), C.byref(ops), C.byref(n)))
    prog = np.frombuffer(C.string_at(ops, n.value * OP_DTYPE.itemsize), dtype=OP_DTYPE).copy()
    _lib.lib().rv_free(ops)
    return prog


def dumps(prog) -> bytes:
    """rv_op array (or list of op tuples) -> bincode bytes"""
    prog = program(prog)
    out = C.c_void_p()
    n = C.c_size_t()
    _lib.check(_lib.lib().rv_program_to_bincode(prog.ctypes.data_as(C.c_void_p), C.c_size_t(len(prog)), C.byref(out), C.byref(n)))
    data = C.string_at(out, n.value)
    _lib.lib().rv_free(out)
    return data


_RV_E_ARG = 9
_EMPTY = np.zeros(1, np.uint8)  # (an address for empty input: the library wants a pointer)


def _context(device):
    from .proof import Context

    return device if isinstance(device, Context) else Context.default() if device is None else Context(int(device))


def loads_device(data, device=None):
    """-> (ops, info): `loads` on the GPU (rv_program_from_bincode_device).  ops is a torch uint8 tensor of shape [n_ops, 24] in GPU
    memory holding exactly the records `loads` returns -- what `Circuit.from_device_ops`, `compact_wires` and the `reverie_amd.stream`
    entry points take as it is.  info: rv_program_info's fields (n_ops, bytes, z64_wires, gf2_wires, n_gf2, n_z64, n_b2a, n_sizehint)
    and wire_counts = (z64_wires, gf2_wires), what `ops.largest_wires` returns for the records.  data: bytes, any buffer (an mmap, a
    uint8 numpy array: passed without a copy; the library uploads it) or a torch uint8 tensor in GPU memory (parsed where it lies).
    device: a `Context` or a device index (None: the default context).  Errors are `loads`', for every byte string."""
    import torch

    from .bristol import _host_buffer
    from .proof import _is_device_ops

    ctx = _context(device)
    L = _lib.lib()
    on_device = _is_device_ops(data)
    if on_device:
        if data.device.type != "cuda" or data.dtype != torch.uint8 or not data.is_contiguous():
            raise ValueError("a tensor of file bytes must be a contiguous uint8 tensor in GPU memory")
        if data.device.index is not None and data.device.index != ctx.device:
            raise ValueError(f"the data is on {data.device}, the context on device {ctx.device}")
        torch.cuda.synchronize(data.device)
        n_data, p_data = data.numel(), data.data_ptr() if data.numel() else _EMPTY.ctypes.data
        on_device = bool(data.numel())
    else:
        buf = _host_buffer(data)
        n_data, p_data = buf.size, buf.ctypes.data if buf.size else _EMPTY.ctypes.data
    info, n = _lib.ProgramInfo(), C.c_size_t()

    def call(ops, cap):
        return L.rv_program_from_bincode_device(ctx.handle, C.c_void_p(p_data), C.c_size_t(n_data), C.c_int(1 if on_device else 0),
                                                C.c_void_p(ops.data_ptr()) if ops is not None else None, C.c_size_t(cap), C.byref(n), C.byref(info))

    dev = torch.device("cuda", ctx.device)
    rc = call(None, 0)  # the sizing call: validates, counts
    ops = torch.empty((0, OP_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    if rc == _RV_E_ARG and n.value:
        ops = torch.empty((int(n.value), OP_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        rc = call(ops, int(n.value))
    _lib.check(rc)
    d = {k: int(getattr(info, k)) for k, _ in info._fields_}
    d["wire_counts"] = (d["z64_wires"], d["gf2_wires"])
    return ops[:int(n.value)], d


def dumps_device(ops, device=None):
    """an op tensor (torch uint8 [n_ops, 24] in GPU memory) -> the bytes `dumps` writes for its records, as a torch uint8 tensor in
    GPU memory (rv_program_to_bincode_device)"""
    import torch

    from .proof import _is_device_ops

    if not _is_device_ops(ops) or ops.device.type != "cuda" or ops.dtype != torch.uint8 or not ops.is_contiguous() or ops.numel() % OP_DTYPE.itemsize:
        raise ValueError("dumps_device takes a contiguous uint8 tensor of 24-byte rv_op records in GPU memory")
    ctx = _context(device)
    if ops.device.index is not None and ops.device.index != ctx.device:
        raise ValueError(f"the ops are on {ops.device}, the context on device {ctx.device}")
    torch.cuda.synchronize(ops.device)
    L = _lib.lib()
    n_ops = ops.numel() // OP_DTYPE.itemsize
    p_ops = C.c_void_p(ops.data_ptr()) if n_ops else None
    n = C.c_size_t()
    rc = L.rv_program_to_bincode_device(ctx.handle, p_ops, C.c_size_t(n_ops), None, C.c_size_t(0), C.byref(n))
    if rc != _RV_E_ARG or not n.value:  # (a sizing call answers RV_E_ARG with the size; anything else is the records' own code)
        _lib.check(rc or _RV_E_ARG)
    out = torch.empty(int(n.value), dtype=torch.uint8, device=torch.device("cuda", ctx.device))
    _lib.check(L.rv_program_to_bincode_device(ctx.handle, p_ops, C.c_size_t(n_ops), C.c_void_p(out.data_ptr()), C.c_size_t(out.numel()), C.byref(n)))
    return out[:int(n.value)]
