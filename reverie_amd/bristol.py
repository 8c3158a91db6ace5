"""Bristol / Bristol Fashion front end: text -> rv_op program, on the host (`parse`) or on the GPU (`parse_device`).

The reference README advertises Bristol-format circuits but leaves parsing to the
un-vendored `mcircuit` crate (/root/reference/README.md:14-16, src/lib.rs:6-7).  The
parser itself is C++ behind the C-ABI (`rv_bristol_parse`, reverie_amd/csrc/bristol.cpp) and, for a program that is to be made in
GPU memory, kernels behind it (`rv_bristol_parse_device`, reverie_amd/csrc/bristol_dev.hip: DESIGN §18); this is the ctypes wrapper.
`dumps` writes a GF(2) program of Bristol shape back as Fashion text, in numpy; `dumps_host` (rv_bristol_write), `dumps_device`
(rv_bristol_write_device) and `DeviceWriter` / `write_device` (rv_bristol_writer_*: the list handed over in pieces) write the same
bytes through the library, on the host and on the GPU (reverie_amd/csrc/bristol_write.h, bristol_write.hip: DESIGN §20).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .ops import OP_DTYPE
from .program_file import _WindowWriter


def parse(text: str | bytes, expected_outputs: Optional[Sequence[int]] = None, fmt: int = 0, compact: bool = False) -> Tuple[np.ndarray, dict]:
    """-> (program, info).  With expected_outputs the program ends with one AddConst+AssertZero
    per output wire, i.e. it states "this witness drives the circuit to these outputs".
    info["wire_counts"] is the (z64, gf2) tuple Proof.new / Proof.verify take.  A wrong number of expected outputs
    is RV_E_ARG (checked by the parser before it reads any of them).
    compact: Bristol files are in SSA form (a wire per gate); with compact=True the program comes back renumbered by liveness
    (rv_ops_compact_wires: the same proof, wire counts sized by the live values -- what a stream's wire store wants), in place of
    the parser's numbering: info["wire_counts"] / info["gf2_wires"] are the new counts, info["ssa_wire_counts"] the parser's and
    info["compact"] is rv_compact_info."""
    data = text.encode() if isinstance(text, str) else bytes(text)
    exp = None
    if expected_outputs is not None:
        exp = np.ascontiguousarray(np.asarray(expected_outputs, dtype=np.uint8))
    ops = C.c_void_p()
    n = C.c_size_t()
    info = _lib.BristolInfo()
    _lib.check(_lib.lib().rv_bristol_parse(data, C.c_size_t(len(data)), C.c_int(fmt),
                                           exp.ctypes.data_as(C.c_void_p) if exp is not None else None,
                                           C.c_size_t(len(exp) if exp is not None else 0),
                                           C.byref(ops), C.byref(n), C.byref(info)))
    prog = np.frombuffer(C.string_at(ops, n.value * OP_DTYPE.itemsize), dtype=OP_DTYPE).copy()
    _lib.lib().rv_free(ops)
    d = {k: int(getattr(info, k)) for k, _ in info._fields_}
    d["wire_counts"] = (0, d["gf2_wires"])
    if compact:
        from .compact import compact_wires

        prog, wc, cinfo = compact_wires(prog, d["wire_counts"])
        d["ssa_wire_counts"], d["wire_counts"], d["gf2_wires"], d["compact"] = d["wire_counts"], wc, wc[1], cinfo
    return prog, d


def _info_dict(info) -> dict:
    d = {k: int(getattr(info, k)) for k, _ in info._fields_}
    d["wire_counts"] = (0, d["gf2_wires"])
    return d


def header(text, fmt: int = 0) -> Tuple[dict, int]:
    """rv_bristol_header (host only): ({n_gates, n_wires, n_inputs, n_outputs, ...}, offset of the gate lines).  `text` must reach the
    end of the first non-blank gate line."""
    buf = _host_buffer(text)
    info, off = _lib.BristolInfo(), C.c_size_t()
    _lib.check(_lib.lib().rv_bristol_header(C.c_void_p(buf.ctypes.data), C.c_size_t(buf.size), C.c_int(fmt), C.byref(info), C.byref(off)))
    return _info_dict(info), int(off.value)


_RV_E_ARG = 9
_EMPTY = np.zeros(1, np.uint8)  # (an address for an empty text: the parser wants a pointer)


def _host_buffer(text) -> np.ndarray:
    """a uint8 view of a host text, without a copy where the object exports a buffer (bytes, mmap, numpy)"""
    if isinstance(text, str):
        text = text.encode()
    a = np.frombuffer(text, dtype=np.uint8) if not isinstance(text, np.ndarray) else np.ascontiguousarray(text).view(np.uint8).reshape(-1)
    return a if a.size else _EMPTY[:0]


def parse_device(text, expected_outputs: Optional[Sequence[int]] = None, fmt: int = 0, compact: bool = False, device=None):
    """-> (ops, info): `parse` on the GPU (rv_bristol_parse_device).  ops is a torch uint8 tensor of shape [n_ops, 24] in GPU memory
    holding exactly the records `parse` returns -- what `Circuit.from_device_ops`, `compact_wires` and the `reverie_amd.stream` entry
    points take as it is; info has `parse`'s keys.  text: bytes, str, any buffer (an mmap, a uint8 numpy array: passed without a copy;
    the library uploads it) or a torch uint8 tensor in GPU memory (parsed where it lies).  device: a `Context` or a device index (None: the default
    context).  Errors are `parse`'s, for every byte string.
    compact: the tensor goes through `compact_wires` (the device path) and info reports the counts as `parse(..., compact=True)`."""
    import torch

    from .proof import Context, _is_device_ops

    ctx = device if isinstance(device, Context) else Context.default() if device is None else Context(int(device))
    L = _lib.lib()
    on_device = _is_device_ops(text)
    if on_device:
        if text.device.type != "cuda" or text.dtype != torch.uint8 or not text.is_contiguous():
            raise ValueError("a tensor text must be a contiguous uint8 tensor in GPU memory")
        if text.device.index is not None and text.device.index != ctx.device:
            raise ValueError(f"the text is on {text.device}, the context on device {ctx.device}")
        torch.cuda.synchronize(text.device)
        n_text, p_text = text.numel(), text.data_ptr() if text.numel() else _EMPTY.ctypes.data
        on_device = bool(text.numel())
    else:
        buf = _host_buffer(text)
        n_text, p_text = buf.size, buf.ctypes.data if buf.size else _EMPTY.ctypes.data
    exp = None
    if expected_outputs is not None:
        exp = np.ascontiguousarray(np.asarray(expected_outputs, dtype=np.uint8))
    p_exp = exp.ctypes.data if exp is not None and exp.size else (_EMPTY.ctypes.data if exp is not None else None)
    n_exp = len(exp) if exp is not None else 0
    info, n = _lib.BristolInfo(), C.c_size_t()

    def call(ops, cap):
        return L.rv_bristol_parse_device(ctx.handle, C.c_void_p(p_text), C.c_size_t(n_text), C.c_int(1 if on_device else 0), C.c_int(fmt),
                                         C.c_void_p(p_exp) if p_exp is not None else None, C.c_size_t(n_exp),
                                         C.c_void_p(ops.data_ptr()) if ops is not None and cap else None, C.c_size_t(cap), C.byref(n), C.byref(info))

    dev = torch.device("cuda", ctx.device)
    if on_device:
        ops, cap = None, 0  # (the header is in GPU memory: the first call sizes)
    else:
        # exact unless the text has MAND lines of several lanes; a header error is the parser's to report
        h, off = _lib.BristolInfo(), C.c_size_t()
        cap = 0
        if L.rv_bristol_header(C.c_void_p(p_text), C.c_size_t(n_text), C.c_int(fmt), C.byref(h), C.byref(off)) == _lib.RV_OK:
            cap = int(h.n_inputs) + int(h.n_gates) + 2 * n_exp
            if cap > n_text + 4096:  # (more records than the text can justify, inputs a header merely claims: a sizing call first)
                cap = 0
        ops = torch.empty((cap, OP_DTYPE.itemsize), dtype=torch.uint8, device=dev) if cap else None
    rc = call(ops, cap)
    if rc == _RV_E_ARG and (ops is None or n.value > cap):
        # the capacity answer: *n_ops is the count (an argument error proper answers the second call as it did the first; a text
        # of no record at all still wants an address, so one record's room is the least)
        cap = max(int(n.value), 1)
        ops = torch.empty((cap, OP_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        rc = call(ops, cap)
    _lib.check(rc)
    n_ops = int(n.value)
    out = ops[:n_ops]
    d = _info_dict(info)
    if compact:
        from .compact import compact_wires

        out, wc, cinfo = compact_wires(out, d["wire_counts"], ctx)
        d["ssa_wire_counts"], d["wire_counts"], d["gf2_wires"], d["compact"] = d["wire_counts"], wc, wc[1], cinfo
    return out, d


def dumps(prog, n_outputs: int = 0) -> bytes:
    """A GF(2) rv_op program of Bristol shape as Bristol Fashion text (host only): the leading Input ops are wires 0 .. n_in - 1 in
    order, then Add -> XOR, Mul -> AND, AddConst 1 -> INV, AddConst 0 -> EQW, Const -> EQ, one line each; the wire count is the
    largest index named plus one, n_outputs the header's output count (the last wires).  Any other op (another domain, Sub, Random,
    AssertZero, ...) raises ValueError.  parse(dumps(p)) returns p."""
    from .ops import program

    p = program(prog) if len(prog) else np.zeros(0, OP_DTYPE)
    is_in = (p["domain"] == 0) & (p["opcode"] == 0)
    n_in = int(np.argmin(is_in)) if not is_in.all() else len(p)
    if (p["domain"] != 0).any() or is_in[n_in:].any() or (p["dst"][:n_in] != np.arange(n_in)).any():
        raise ValueError("dumps takes a GF(2) program whose Input ops lead it, on wires 0 .. n_in - 1 in order")
    g = p[n_in:]
    opc, imm = g["opcode"], g["imm"]
    if (g["reserved"] != 0).any() or (p["reserved"][:n_in] != 0).any():
        raise ValueError("reserved must be 0")
    two = (opc == 2) | (opc == 6)
    one = opc == 3
    const = opc == 9
    if not (two | one | const).all() or (imm[one | const] > 1).any():
        raise ValueError("dumps writes Add, Mul, AddConst 0/1 and Const 0/1 only")
    n_wires = int(max(n_in, int(p["dst"].max(initial=0)) + 1 if len(p) else 0, int(g["a"][two | one].max(initial=0)) + 1 if (two | one).any() else 0,
                      int(g["b"][two].max(initial=0)) + 1 if two.any() else 0))
    if n_outputs > n_wires:
        raise ValueError("more outputs than wires")
    head = b"%d %d\n1 %d\n1 %d\n\n" % (len(g), n_wires, n_in, n_outputs)
    if not len(g):
        return head
    # every line is laid out by arithmetic on whole columns: the digit counts give the line lengths, their running sum the line starts,
    # and each decimal position of each number column is one masked scatter into the text
    x = np.where(const, imm, g["a"]).astype(np.int64)  # the first number: operand a, or EQ's literal
    y, z = g["b"].astype(np.int64), g["dst"].astype(np.int64)
    nd = lambda v: 1 + sum((v >= 10 ** k).astype(np.int64) for k in range(1, 10))  # noqa: E731
    nx, ny, nz = nd(x), np.where(two, nd(y) + 1, 0), nd(z)
    klen = np.where(const, 2, 3)
    length = 4 + nx + 1 + ny + nz + 1 + klen + 1
    start = np.cumsum(length) - length
    buf = np.full(int(length.sum()), ord(" "), np.uint8)
    buf[start] = np.where(two, ord("2"), ord("1"))
    buf[start + 2] = ord("1")
    buf[start + length - 1] = ord("\n")

    def put(v, n, at, mask=None):
        for k in range(10):
            m = n > k if mask is None else mask & (n > k)
            if not m.any():
                break
            buf[at[m] + n[m] - 1 - k] = 48 + (v[m] // 10 ** k) % 10

    px = start + 4
    put(x, nx, px)
    put(y, ny - 1, px + nx + 1, two)
    pz = px + nx + 1 + ny
    put(z, nz, pz)
    kinds = np.zeros((len(g), 3), np.uint8)
    for sel, name in ((opc == 2, b"XOR"), (opc == 6, b"AND"), (one & (imm == 1), b"INV"), (one & (imm == 0), b"EQW"), (const, b"EQ\n")):
        kinds[sel] = np.frombuffer(name, np.uint8)
    pk = pz + nz + 1
    for k in range(3):
        buf[pk + k] = kinds[:, k]
    return head + buf.tobytes()


# ---- a text read in windows (rv_bristol_reader_*) ----
def _expected(expected_outputs):
    """(array or None, address or None, count) of the expected outputs, as the C calls take them"""
    if expected_outputs is None:
        return None, None, 0
    exp = np.ascontiguousarray(np.asarray(expected_outputs, dtype=np.uint8))
    return exp, (exp.ctypes.data if exp.size else _EMPTY.ctypes.data), int(exp.size)


class DeviceReader:
    """`parse_device` for a text that is handed over in windows: consecutive byte ranges of any length (rv_bristol_reader_*).  Neither
    the text nor its records are ever whole in memory, and file_len may be 2^32 and more (one window stays below 2^32 bytes).

        with DeviceReader(file_len, expected_outputs) as r:
            for window in windows: ops, piece = r.feed(window)    # the records of the gate lines that are now complete
            info = r.finish()                                     # parse_device's info, for the whole text

    The records of all feeds, in order, are exactly `parse`'s records for the whole text, and the first error raised is `parse`'s
    error, for every byte string and every way of cutting it; afterwards the reader takes nothing more.  The Input ops come with the
    feed that completes the header, the assertion pairs with the feed that completes the last gate line; bytes behind that line are
    never judged and need not be fed."""

    def __init__(self, file_len: int, expected_outputs: Optional[Sequence[int]] = None, fmt: int = 0, device=None):
        from .proof import Context

        self.ctx = device if isinstance(device, Context) else Context.default() if device is None else Context(int(device))
        self.handle = C.c_void_p()
        exp, p_exp, self.n_expected = _expected(expected_outputs)
        _lib.check(_lib.lib().rv_bristol_reader_begin(self.ctx.handle, C.c_uint64(int(file_len)), C.c_int(fmt),
                                                      C.c_void_p(p_exp) if p_exp is not None else None, C.c_size_t(self.n_expected), C.byref(self.handle)))

    def feed(self, data, scan: bool = False, out=None):
        """-> (ops, piece).  data: bytes, any buffer (an mmap or a slice of one, a uint8 numpy array) or a uint8 torch tensor in GPU
        memory (a slice of a larger one is fine; no alignment is asked).  ops: a torch uint8 tensor [n, 24] in GPU memory; scan=True:
        None -- nothing is written, the piece and the info are complete all the same.  piece: first_op, n_ops, n_input_gf2 (what a
        stream feed of these records takes from the witness; n_input_z64 is 0), first_line, n_lines.  out: a uint8 GPU tensor to
        write into instead of a new one.  Where the buffer is too small for the feed -- len(data) // 6 + 1 records are tried first, a
        header's inputs and pairs and a line carried over can ask for more -- the same bytes are fed again with the count the
        library names (rv_stream_finish_device's rule)."""
        import torch

        from .proof import _is_device_ops

        on_device = _is_device_ops(data)
        if on_device:
            if data.device.type != "cuda" or data.dtype != torch.uint8 or not data.is_contiguous():
                raise ValueError("a tensor of text bytes must be a contiguous uint8 tensor in GPU memory")
            if data.device.index is not None and data.device.index != self.ctx.device:
                raise ValueError(f"the data is on {data.device}, the context on device {self.ctx.device}")
            torch.cuda.synchronize(data.device)
            n_data, p_data = data.numel(), data.data_ptr() if data.numel() else _EMPTY.ctypes.data
            on_device = bool(data.numel())
        else:
            buf = _host_buffer(data)
            n_data, p_data = buf.size, buf.ctypes.data if buf.size else _EMPTY.ctypes.data
        piece = _lib.BristolPiece()

        def call(ops, cap):
            return _lib.lib().rv_bristol_reader_feed(self.handle, C.c_void_p(p_data), C.c_size_t(n_data), C.c_int(1 if on_device else 0),
                                                     C.c_void_p(ops.data_ptr()) if ops is not None else None, C.c_size_t(cap), C.byref(piece))

        ops = None
        if scan:
            _lib.check(call(None, 0))
        else:
            dev = torch.device("cuda", self.ctx.device)
            if out is None:
                out = torch.empty((n_data // 6 + 1, OP_DTYPE.itemsize), dtype=torch.uint8, device=dev)
            elif not _is_device_ops(out) or out.device.type != "cuda" or out.dtype != torch.uint8 or not out.is_contiguous():
                raise ValueError("out must be a contiguous uint8 tensor in GPU memory")
            ops, cap = out.reshape(-1, OP_DTYPE.itemsize), out.numel() // OP_DTYPE.itemsize
            rc = call(ops, cap)
            if rc == _RV_E_ARG and int(piece.n_ops) > cap:  # the capacity answer: the reader has not moved
                cap = int(piece.n_ops)
                ops = torch.empty((cap, OP_DTYPE.itemsize), dtype=torch.uint8, device=dev)
                rc = call(ops, cap)
            _lib.check(rc)
        d = {k: int(getattr(piece, k)) for k, _ in piece._fields_}
        d["n_input_z64"] = 0
        return (ops[:d["n_ops"]] if ops is not None else None), d

    def header(self) -> dict:
        """the header's counts (n_gates, n_wires, n_inputs, n_outputs, gf2_wires, wire_counts) once the header is in (an error before)"""
        info = _lib.BristolInfo()
        _lib.check(_lib.lib().rv_bristol_reader_header(self.handle, C.byref(info)))
        return _info_dict(info)

    def finish(self) -> dict:
        """`parse_device`'s info for the whole text, once the gate lines the header counts and the pairs are out (an error before)"""
        info = _lib.BristolInfo()
        _lib.check(_lib.lib().rv_bristol_reader_finish(self.handle, C.byref(info)))
        return _info_dict(info)

    def close(self):
        if self.handle:
            if self.ctx.handle:
                _lib.lib().rv_bristol_reader_destroy(self.handle)
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


def iter_device(source, window_bytes: int = 64 << 20, expected_outputs: Optional[Sequence[int]] = None, fmt: int = 0, device=None, scan: bool = False,
                info=None):
    """The Bristol text `source` -- a path (memory-mapped), a buffer or a uint8 torch tensor in GPU memory -- read in windows of
    window_bytes: yields `DeviceReader.feed`'s (ops, piece) per window, windows that complete no line included.  Device memory is
    one window, its work memory and its records, whatever the text's length.  info: a dict that receives `finish`'s info at the
    end."""
    from .program_file import _window_source

    window_bytes = int(window_bytes)
    if not 0 < window_bytes < 1 << 32:
        raise ValueError("window_bytes must be in [1, 2^32)")
    data, n = _window_source(source)
    with DeviceReader(n, expected_outputs, fmt, device) as r:
        for at in range(0, max(n, 1), window_bytes):
            yield r.feed(data[at:at + window_bytes], scan=scan)
        done = r.finish()
        if info is not None:
            info.update(done)


def head_info(source, fmt: int = 0) -> dict:
    """the header's counts (n_gates, n_wires, n_inputs, n_outputs; the rest 0) of a Bristol text, from the head of `source` (a path, a
    buffer or a uint8 GPU tensor) alone: rv_bristol_header_prefix on the first bytes that hold four non-blank lines.  Errors are the
    header's."""
    from .program_file import _window_source

    data, n = _window_source(source)
    take = min(n, 4096)
    while True:
        head = data[:take]
        head = _host_buffer(head.cpu().numpy() if hasattr(head, "cpu") else head)
        lines, token = 0, False
        for c in head.tobytes():
            if c == 10:
                lines, token = lines + token, False
            elif c not in (32, 9, 13):
                token = True
            if lines >= 4:
                break
        if lines >= 4 or take == n:
            break
        take = min(n, take * 2)
    bi, off = _lib.BristolInfo(), C.c_size_t()
    _lib.check(_lib.lib().rv_bristol_header_prefix(C.c_void_p(head.ctypes.data if head.size else _EMPTY.ctypes.data), C.c_size_t(head.size), C.c_uint64(n),
                                                   C.c_int(fmt), C.byref(bi), C.byref(off)))
    return {k: int(getattr(bi, k)) for k, _ in bi._fields_}


def wire_counts(source, expected_outputs: Optional[Sequence[int]] = None, fmt: int = 0) -> Tuple[int, int]:
    """(0, gf2_wires) of a Bristol text -- what a stream over `iter_device` begins with -- from the head of `source` (a path, a buffer
    or a uint8 GPU tensor) alone: rv_bristol_header_prefix on the first bytes that hold four non-blank lines.  No pass over the text:
    the header names the wires, and the assertion temporaries are one per expected output.  Errors are the header's."""
    exp, _, n_exp = _expected(expected_outputs)
    bi = head_info(source, fmt)
    if exp is not None and n_exp != bi["n_outputs"]:
        _lib.check(_RV_E_ARG)
    return 0, bi["n_wires"] + (n_exp if exp is not None else 0)


# ---- Bristol text written on the GPU, whole and in windows (rv_bristol_write*) ----
def dumps_host(prog, n_outputs: int = 0, n_wires: Optional[int] = None) -> bytes:
    """`dumps` by the library's host writer (rv_bristol_write, no GPU): the same bytes, and a ReverieError where `dumps` raises
    ValueError.  n_wires: the header's wire count (None: derived, as `dumps` derives it)."""
    from .ops import program

    p = program(prog) if len(prog) else np.zeros(0, OP_DTYPE)
    out, n = C.c_void_p(), C.c_size_t()
    _lib.check(_lib.lib().rv_bristol_write(C.c_void_p(p.ctypes.data) if len(p) else None, C.c_size_t(len(p)), C.c_uint64(int(n_wires or 0)),
                                           C.c_uint64(int(n_outputs)), C.byref(out), C.byref(n)))
    data = C.string_at(out, n.value)
    _lib.lib().rv_free(out)
    return data


def dumps_device(ops, n_outputs: int = 0, n_wires: Optional[int] = None, device=None):
    """an op tensor in GPU memory (packed rv_op records) -> the bytes `dumps` writes for its records, as a torch uint8 tensor in GPU
    memory (rv_bristol_write_device: a sizing call, then the write).  Errors are rv_bristol_write's."""
    import torch

    from .proof import Context, _device_ops

    ctx = device if isinstance(device, Context) else Context.default() if device is None else Context(int(device))
    d_ops, n_ops, _ = _device_ops(ops, ctx, "dumps_device")
    L = _lib.lib()
    p_ops = C.c_void_p(d_ops) if n_ops else None
    args = (ctx.handle, p_ops, C.c_size_t(n_ops), C.c_uint64(int(n_wires or 0)), C.c_uint64(int(n_outputs)))
    n = C.c_size_t()
    rc = L.rv_bristol_write_device(*args, None, C.c_size_t(0), C.byref(n))
    if rc != _RV_E_ARG or not n.value:  # (a sizing call answers RV_E_ARG with the size; anything else is the records' own code)
        _lib.check(rc or _RV_E_ARG)
    out = torch.empty(int(n.value), dtype=torch.uint8, device=torch.device("cuda", ctx.device))
    _lib.check(L.rv_bristol_write_device(*args, C.c_void_p(out.data_ptr()), C.c_size_t(out.numel()), C.byref(n)))
    return out[:int(n.value)]


class DeviceWriter(_WindowWriter):
    """`dumps_device` for an op list that is handed over in pieces (rv_bristol_writer_*): the bytes of all feeds, in order, are
    `dumps`' bytes for the whole list, however it is cut; the first feed's begin with the header lines.  The header goes out
    first, so the writer is told what `dumps` derives: n_inputs (the leading Input records) and n_wires.

        with DeviceWriter(n_ops, n_inputs, n_wires, n_outputs) as w:
            for ops in pieces: text, piece = w.feed(ops)
            w.finish()"""

    _FEED, _FINISH, _DESTROY = "rv_bristol_writer_feed", "rv_bristol_writer_finish", "rv_bristol_writer_destroy"
    _HEAD, _PER_OP = 96, 41

    def __init__(self, n_ops: int, n_inputs: int, n_wires: int, n_outputs: int = 0, device=None):
        from .program_file import _context

        self.ctx = _context(device)
        self.handle = C.c_void_p()
        _lib.check(_lib.lib().rv_bristol_writer_begin(self.ctx.handle, C.c_uint64(int(n_ops)), C.c_uint64(int(n_inputs)), C.c_uint64(int(n_wires)),
                                                      C.c_uint64(int(n_outputs)), C.byref(self.handle)))


def write_device(pieces, dst, n_ops: int, n_inputs: int, n_wires: int, n_outputs: int = 0, device=None) -> int:
    """Writes the Bristol text of an op list that comes in pieces -- an iterator of op pieces; tuples of (ops, anything), as
    `iter_device` and `compact.compact_pieces` yield them, are taken as they are -- to dst, a path or a binary file object: one feed,
    one copy to the host and one write per piece.  -> the bytes written."""
    from .program_file import _write_pieces

    return _write_pieces(DeviceWriter(n_ops, n_inputs, n_wires, n_outputs, device), pieces, dst)
