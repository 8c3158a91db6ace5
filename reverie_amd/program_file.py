"""Program files of the reference CLI: bincode(`Vec<mcircuit::CombineOperation>`), read at
/root/reference/src/main.rs:66,98,122.  The (de)serialiser is C++ behind the C-ABI
(`rv_program_from_bincode` / `rv_program_to_bincode`, reverie_amd/csrc/program.cpp); this is the ctypes
wrapper.  The enum's variant order is recalled, not verifiable here — see the header.
`loads_device` / `dumps_device` are the same two on the GPU (`rv_program_from_bincode_device` / `rv_program_to_bincode_device`,
reverie_amd/csrc/bincode_dev.hip: DESIGN §19): the op list is made in, and written from, device memory.  `DeviceReader` / `iter_device` /
`scan_device` read a file in windows (`rv_program_reader_*`): for files no memory holds whole.  `DeviceWriter` /
`write_device` write one from an op list that is handed over in pieces (`rv_program_writer_*`)."""
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


# ---- a file read in windows (rv_program_reader_*) ----
def _info_dict(info) -> dict:
    d = {k: int(getattr(info, k)) for k, _ in info._fields_}
    d["wire_counts"] = (d["z64_wires"], d["gf2_wires"])
    return d


class DeviceReader:
    """`loads_device` for a file that is handed over in windows: consecutive byte ranges of any length (rv_program_reader_*).  Neither
    the file nor its records are ever whole in memory, and file_len may be 2^32 and more (one window stays below 2^32 bytes).

        with DeviceReader(file_len) as r:
            for window in windows: ops, piece = r.feed(window)    # the records whose last byte has now been fed
            info = r.finish()                                     # loads_device's info, for the whole file

    The records of all feeds, in order, are exactly `loads`' records for the whole file, and the first error raised is `loads`'
    error, for every byte string and every way of cutting it; afterwards the reader takes nothing more.  Bytes behind the last
    record the header counts are never judged and need not be fed."""

    def __init__(self, file_len: int, device=None):
        self.ctx = _context(device)
        self.handle = C.c_void_p()
        _lib.check(_lib.lib().rv_program_reader_begin(self.ctx.handle, C.c_uint64(int(file_len)), C.byref(self.handle)))

    def feed(self, data, scan: bool = False, out=None):
        """-> (ops, piece).  data: bytes, any buffer (an mmap or a slice of one, a uint8 numpy array) or a uint8 torch tensor in GPU
        memory (a slice of a larger one is fine; no alignment is asked).  ops: a torch uint8 tensor [n, 24] in GPU memory; scan=True:
        None -- nothing is written, the piece and the info are complete all the same.  piece: first_op, n_ops, n_input_gf2,
        n_input_z64 (what a stream feed of these records takes from the witness).  out: a uint8 GPU tensor with room for
        len(data) // 16 + 1 records to write into instead of a new one."""
        import torch

        from .bristol import _host_buffer
        from .proof import _is_device_ops

        on_device = _is_device_ops(data)
        if on_device:
            if data.device.type != "cuda" or data.dtype != torch.uint8 or not data.is_contiguous():
                raise ValueError("a tensor of file bytes must be a contiguous uint8 tensor in GPU memory")
            if data.device.index is not None and data.device.index != self.ctx.device:
                raise ValueError(f"the data is on {data.device}, the context on device {self.ctx.device}")
            torch.cuda.synchronize(data.device)
            n_data, p_data = data.numel(), data.data_ptr() if data.numel() else _EMPTY.ctypes.data
            on_device = bool(data.numel())
        else:
            buf = _host_buffer(data)
            n_data, p_data = buf.size, buf.ctypes.data if buf.size else _EMPTY.ctypes.data
        ops, cap = None, n_data // 16 + 1
        if not scan:
            if out is None:
                out = torch.empty((cap, OP_DTYPE.itemsize), dtype=torch.uint8, device=torch.device("cuda", self.ctx.device))
            elif not _is_device_ops(out) or out.device.type != "cuda" or out.dtype != torch.uint8 or not out.is_contiguous():
                raise ValueError("out must be a contiguous uint8 tensor in GPU memory")
            ops, cap = out.reshape(-1, OP_DTYPE.itemsize), out.numel() // OP_DTYPE.itemsize
        piece = _lib.ProgramPiece()
        _lib.check(_lib.lib().rv_program_reader_feed(self.handle, C.c_void_p(p_data), C.c_size_t(n_data), C.c_int(1 if on_device else 0),
                                                     C.c_void_p(ops.data_ptr()) if ops is not None else None, C.c_size_t(cap if ops is not None else 0),
                                                     C.byref(piece)))
        d = {k: int(getattr(piece, k)) for k, _ in piece._fields_}
        return (ops[:d["n_ops"]] if ops is not None else None), d

    def finish(self) -> dict:
        """`loads_device`'s info for the whole file, once the records the header counts are out (an error before that)"""
        info = _lib.ProgramInfo()
        _lib.check(_lib.lib().rv_program_reader_finish(self.handle, C.byref(info)))
        return _info_dict(info)

    def close(self):
        if self.handle:
            if self.ctx.handle:
                _lib.lib().rv_program_reader_destroy(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _window_source(source):
    """(something to slice by bytes, its length) of a path (memory-mapped), a buffer or a uint8 GPU tensor"""
    import os

    from .bristol import _host_buffer
    from .proof import _is_device_ops

    if _is_device_ops(source):
        return source.reshape(-1), source.numel()
    if isinstance(source, (str, os.PathLike)):
        size = os.path.getsize(source)
        return (np.memmap(source, dtype=np.uint8, mode="r") if size else _EMPTY[:0]), size  # (an empty file cannot be mapped)
    buf = _host_buffer(source)
    return buf, buf.size


def iter_device(source, window_bytes: int = 64 << 20, device=None, scan: bool = False, info=None):
    """The program file `source` -- a path (memory-mapped), a buffer or a uint8 torch tensor in GPU memory -- read in windows of
    window_bytes: yields `DeviceReader.feed`'s (ops, piece) per window, windows that complete no record included.  Device memory
    is one window, its work memory and its records, whatever the file's length.  info: a dict that receives `finish`'s info at the
    end."""
    window_bytes = int(window_bytes)
    if not 0 < window_bytes < 1 << 32:
        raise ValueError("window_bytes must be in [1, 2^32)")
    data, n = _window_source(source)
    with DeviceReader(n, device) as r:
        for at in range(0, max(n, 1), window_bytes):
            yield r.feed(data[at:at + window_bytes], scan=scan)
        done = r.finish()
        if info is not None:
            info.update(done)


def scan_device(source, window_bytes: int = 64 << 20, device=None) -> dict:
    """`loads_device`'s info of a file read in windows, nothing written: the pre-pass that gives a stream its wire counts"""
    info = {}
    for _ in iter_device(source, window_bytes, device, scan=True, info=info):
        pass
    return info


# ---- a file written in windows (rv_program_writer_*) ----
class _WindowWriter:
    """what `program_file.DeviceWriter` and `bristol.DeviceWriter` share: feeds of op pieces, each answered with its bytes"""

    _FEED, _FINISH, _DESTROY = "", "", ""
    _HEAD, _PER_OP = 0, 0  # head + per_op * n bytes always hold a feed of n records

    def feed(self, ops, out=None):
        """-> (bytes, piece).  ops: an OP_DTYPE array (uploaded by the library) or a torch tensor of packed rv_op records in GPU memory,
        as `DeviceCompactor.feed` takes them.  bytes: a torch uint8 tensor in GPU memory, the feed's part of the output (the first
        feed's begins with the header); piece: first_op, n_ops, file_off, bytes.  out: a uint8 GPU tensor to write into instead of a
        new one; where it is too small the same records are fed again into a new one of the size the library names."""
        import torch

        from .proof import _device_ops, _is_device_ops, _ptr

        if _is_device_ops(ops):
            d_ops, n, _ = _device_ops(ops, self.ctx, type(self).__name__)
            p, dev = C.c_void_p(d_ops) if n else None, 1
        else:
            a = program(ops) if len(ops) else np.zeros(0, OP_DTYPE)
            p, n, dev = _ptr(a), len(a), 0
        if out is None:
            out = torch.empty(self._HEAD + self._PER_OP * n, dtype=torch.uint8, device=torch.device("cuda", self.ctx.device))
        elif not _is_device_ops(out) or out.device.type != "cuda" or out.dtype != torch.uint8 or not out.is_contiguous():
            raise ValueError("out must be a contiguous uint8 tensor in GPU memory")
        piece = _lib.WriterPiece()
        call = getattr(_lib.lib(), self._FEED)
        rc = call(self.handle, p, C.c_size_t(n), C.c_int(dev), C.c_void_p(out.data_ptr()), C.c_size_t(out.numel()), C.byref(piece))
        if rc == _RV_E_ARG and int(piece.bytes) > out.numel():  # the capacity answer: the writer has not moved
            out = torch.empty(int(piece.bytes), dtype=torch.uint8, device=out.device)
            rc = call(self.handle, p, C.c_size_t(n), C.c_int(dev), C.c_void_p(out.data_ptr()), C.c_size_t(out.numel()), C.byref(piece))
        _lib.check(rc)
        d = {k: int(getattr(piece, k)) for k, _ in piece._fields_}
        return out.reshape(-1)[:d["bytes"]], d

    def finish(self) -> None:
        """an error unless the header and exactly n_ops records are out"""
        _lib.check(getattr(_lib.lib(), self._FINISH)(self.handle))

    def close(self):
        if self.handle:
            if self.ctx.handle:
                getattr(_lib.lib(), self._DESTROY)(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceWriter(_WindowWriter):
    """`dumps_device` for an op list that is handed over in pieces (rv_program_writer_*): the bytes of all feeds, in order, are `dumps`'
    bytes for the whole list, however it is cut; the first feed's begin with the 8-byte count.  n_ops may be 2^32 and more.

        with DeviceWriter(n_ops) as w:
            for ops in pieces: data, piece = w.feed(ops)
            w.finish()"""

    _FEED, _FINISH, _DESTROY = "rv_program_writer_feed", "rv_program_writer_finish", "rv_program_writer_destroy"
    _HEAD, _PER_OP = 8, 32

    def __init__(self, n_ops: int, device=None):
        self.ctx = _context(device)
        self.handle = C.c_void_p()
        _lib.check(_lib.lib().rv_program_writer_begin(self.ctx.handle, C.c_uint64(int(n_ops)), C.byref(self.handle)))


def _write_pieces(writer, pieces, dst) -> int:
    """every piece through writer.feed, its bytes copied to the host and written to dst (a path or a binary file object) -> the count"""
    import os

    own = isinstance(dst, (str, os.PathLike))
    f = open(dst, "wb") if own else dst
    total, fed = 0, False
    try:
        with writer as w:
            for piece in pieces:
                data, _ = w.feed(piece[0] if isinstance(piece, tuple) else piece)
                f.write(data.cpu().numpy().data)
                total, fed = total + data.numel(), True
            if not fed:  # (no piece at all: the header of an empty list goes out with a feed of 0 records)
                data, _ = w.feed(np.zeros(0, OP_DTYPE))
                f.write(data.cpu().numpy().data)
                total += data.numel()
            w.finish()
    finally:
        if own:
            f.close()
    return total


def write_device(pieces, dst, n_ops: int, device=None) -> int:
    """Writes the program file of an op list that comes in pieces -- an iterator of op pieces; tuples of (ops, anything), as
    `iter_device` and `compact.compact_pieces` yield them, are taken as they are -- to dst, a path or a binary file object: one feed,
    one copy to the host and one write per piece.  n_ops: the whole list's count (the header says it first).  -> the bytes written."""
    return _write_pieces(DeviceWriter(n_ops, device), pieces, dst)
