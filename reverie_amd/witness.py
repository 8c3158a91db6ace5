"""Witness text parser — /root/reference/src/witness.rs:12-60: the file is scanned byte by
byte, '0' and '1' are witness bits, every other byte is ignored.

`parse_witness` is the numpy definition the command line has always used.  The library has the same rule in C (rv_witness_parse /
rv_witness_write: `parse`, `dumps`) and on the GPU (rv_witness_parse_device, rv_witness_reader_*, rv_witness_write_device:
`parse_device`, `parse_device_batch`, `DeviceReader`, `DeviceWindows`, `dumps_device`), so that a witness file reaches a
proof without a host copy of its bits."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

_RV_E_WITNESS_SHORT = 2
_RV_E_ARG = 9
_EMPTY = np.zeros(1, np.uint8)  # (an address for an empty text: the library wants a pointer)


def parse_witness(data: bytes | str) -> np.ndarray:
    if isinstance(data, str):
        data = data.encode()
    a = np.frombuffer(data, dtype=np.uint8)
    keep = (a == 0x30) | (a == 0x31)
    return (a[keep] - 0x30).astype(np.uint8)


def _host_buffer(data) -> np.ndarray:
    """a uint8 view of a host text, without a copy where the object exports a buffer (bytes, mmap, numpy)"""
    if isinstance(data, str):
        data = data.encode()
    a = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    return a if a.size else _EMPTY[:0]


def _context(ctx):
    from .proof import Context

    return ctx if isinstance(ctx, Context) else Context.default() if ctx is None else Context(int(ctx))


def _source(data, ctx, what: str):
    """(address, length, on_device, the object that keeps the bytes alive) of a text or a bit list: a host buffer, or a contiguous
    uint8 torch tensor on the context's device"""
    from .proof import _is_device_ops

    if _is_device_ops(data):
        import torch

        if data.device.type != "cuda" or data.dtype not in (torch.uint8, torch.bool) or not data.is_contiguous():
            raise ValueError(f"{what}: a tensor must be a contiguous uint8 tensor in GPU memory")
        if data.device.index is not None and data.device.index != ctx.device:
            raise ValueError(f"{what}: the data is on {data.device}, the context on device {ctx.device}")
        torch.cuda.synchronize(data.device)
        n = data.numel()
        return (data.data_ptr() if n else _EMPTY.ctypes.data), n, bool(n), data
    buf = _host_buffer(data)
    return (buf.ctypes.data if buf.size else _EMPTY.ctypes.data), buf.size, False, buf


# ---- the host definition in C (no GPU) ----
def parse(data) -> np.ndarray:
    """`parse_witness` by the library's host parser (rv_witness_parse): the same bits, one uint8 per bit.  data: bytes, str or any
    buffer (an mmap, a uint8 numpy array: read without a copy)."""
    buf = _host_buffer(data)
    out, n = np.empty(buf.size, np.uint8), C.c_size_t()
    _lib.check(_lib.lib().rv_witness_parse(C.c_void_p(buf.ctypes.data if buf.size else _EMPTY.ctypes.data), C.c_size_t(buf.size),
                                           C.c_void_p(out.ctypes.data) if out.size else None, C.c_size_t(out.size), C.byref(n)))
    return out[:n.value]


def dumps(bits, line_bits: int = 0) -> bytes:
    """bits as witness text (rv_witness_write, on the host): '0' / '1', a line feed behind every line_bits bits and behind the last
    one (0: one line).  A value above 1 raises ReverieError (RV_E_ARG).  parse(dumps(x)) == x."""
    b = np.ascontiguousarray(np.asarray(bits, dtype=np.uint8)).reshape(-1)
    L, n = _lib.lib(), C.c_size_t()
    args = (C.c_void_p(b.ctypes.data) if b.size else None, C.c_size_t(b.size), C.c_uint64(int(line_bits)))
    _lib.check(L.rv_witness_write(*args, None, C.c_size_t(0), C.byref(n)))
    out = np.empty(n.value, np.uint8)
    _lib.check(L.rv_witness_write(*args, C.c_void_p(out.ctypes.data) if out.size else None, C.c_size_t(out.size), C.byref(n)))
    return out.tobytes()


# ---- on the GPU ----
def parse_device(data, ctx=None, marks=None):
    """`parse` on the GPU (rv_witness_parse_device) -> a torch uint8 tensor in GPU memory holding one byte per bit: what `Proof.new`,
    `Circuit.evaluate` and the `reverie_amd.stream` entry points take as a witness.  data: bytes, str, any buffer (an mmap, a uint8
    numpy array: passed without a copy; the library uploads it) or a uint8 torch tensor in GPU memory (parsed where it lies, a slice of
    a larger one is fine).  ctx: a `Context` or a device index (None: the default context).
    marks: ascending byte positions <= len(data); the result is then (bits, bits_before), bits_before[m] (a uint64 numpy array) = the
    number of bits in data[:marks[m]]."""
    import torch

    ctx = _context(ctx)
    p, n, on_device, keep = _source(data, ctx, "parse_device")
    out = torch.empty(n, dtype=torch.uint8, device=torch.device("cuda", ctx.device))  # (a text holds at most a bit per byte)
    mk = np.ascontiguousarray(np.asarray(marks, dtype=np.uint64)).reshape(-1) if marks is not None else None
    before = np.zeros(mk.size if mk is not None else 0, np.uint64)
    got = C.c_size_t()
    _lib.check(_lib.lib().rv_witness_parse_device(ctx.handle, C.c_void_p(p), C.c_size_t(n), C.c_int(1 if on_device else 0),
                                                  C.c_void_p(out.data_ptr()) if n else None, C.c_size_t(n), C.byref(got),
                                                  C.c_void_p(mk.ctypes.data) if mk is not None and mk.size else None, C.c_size_t(before.size),
                                                  C.c_void_p(before.ctypes.data) if before.size else None))
    del keep
    bits = out[:got.value]
    return bits if marks is None else (bits, before)


def parse_device_batch(texts, ctx=None):
    """B witness texts -> a [B, n] uint8 tensor in GPU memory, what `Proof.new_batch`, `prove_batch_device` and
    `Circuit.evaluate_batch_device` take: the texts are concatenated (skipped bytes make that harmless) and parsed by one
    rv_witness_parse_device call with a mark at every join.  texts: as `parse_device` takes them; if any is a GPU tensor, the
    concatenation is made in GPU memory.  ValueError names the first text whose bit count differs from the first text's."""
    import torch

    from .proof import _is_device_ops

    ctx = _context(ctx)
    texts = list(texts)
    if not texts:
        raise ValueError("parse_device_batch: no texts")
    if any(_is_device_ops(t) for t in texts):
        dev = torch.device("cuda", ctx.device)
        parts = [t.reshape(-1) if _is_device_ops(t) else torch.from_numpy(_host_buffer(t).copy()).to(dev) for t in texts]
        lens = [int(t.numel()) for t in parts]
        whole = torch.cat(parts)
    else:
        parts = [_host_buffer(t) for t in texts]
        lens = [int(t.size) for t in parts]
        whole = np.concatenate(parts) if len(parts) > 1 else parts[0]
    bits, before = parse_device(whole, ctx, marks=np.cumsum(lens, dtype=np.uint64))
    counts = np.diff(np.concatenate([np.zeros(1, np.uint64), before])).astype(np.int64)
    n = int(counts[0])
    if (counts != n).any():
        b = int(np.argmax(counts != n))
        raise ValueError(f"parse_device_batch: text {b} holds {int(counts[b])} bits, text 0 holds {n}")
    return bits.reshape(len(texts), n)


def dumps_device(bits, line_bits: int = 0, ctx=None):
    """`dumps` on the GPU (rv_witness_write_device): a uint8 tensor of bits in GPU memory -> the text as a uint8 tensor in GPU memory"""
    import torch

    ctx = _context(ctx)
    p, n, on_device, keep = _source(bits, ctx, "dumps_device")
    if not on_device and n:
        raise TypeError("dumps_device takes a torch tensor in GPU memory (dumps writes host bits)")
    L, need = _lib.lib(), C.c_size_t()
    args = (ctx.handle, C.c_void_p(p) if n else None, C.c_size_t(n), C.c_uint64(int(line_bits)))
    _lib.check(L.rv_witness_write_device(*args, None, C.c_size_t(0), C.byref(need)))
    out = torch.empty(need.value, dtype=torch.uint8, device=torch.device("cuda", ctx.device))
    if need.value:
        _lib.check(L.rv_witness_write_device(*args, C.c_void_p(out.data_ptr()), C.c_size_t(out.numel()), C.byref(need)))
    del keep
    return out


class DeviceReader:
    """`parse_device` for a text that is handed over in windows: consecutive byte ranges of any length (rv_witness_reader_*).

        with DeviceReader() as r:
            for window in windows: bits = r.feed(window)     # exactly the bits of this window's bytes
            bytes_fed, bits_total = r.finish()

    A text has no records, so nothing is carried between feeds: the reader is `parse_device` per window plus the two totals, which
    may pass 2^32 (one window stays below 2^32 bytes).  It is the way in for a file of 2^32 bytes and more, or one that must not be
    resident."""

    def __init__(self, ctx=None):
        self.ctx = _context(ctx)
        self.handle = C.c_void_p()
        _lib.check(_lib.lib().rv_witness_reader_begin(self.ctx.handle, C.byref(self.handle)))

    def feed(self, data, out=None):
        """-> the bits of data (bytes, a buffer or a uint8 GPU tensor) as a uint8 tensor in GPU memory.  out: a uint8 GPU tensor to
        write into instead of a new one; where it is too small the same bytes are fed again into a new one of the size the library
        names."""
        import torch

        p, n, on_device, keep = _source(data, self.ctx, "DeviceReader.feed")
        dev = torch.device("cuda", self.ctx.device)
        if out is None:
            out = torch.empty(n, dtype=torch.uint8, device=dev)
        elif not hasattr(out, "data_ptr") or out.device.type != "cuda" or out.dtype != torch.uint8 or not out.is_contiguous():
            raise ValueError("out must be a contiguous uint8 tensor in GPU memory")
        got = C.c_size_t()

        def call(t):
            return _lib.lib().rv_witness_reader_feed(self.handle, C.c_void_p(p), C.c_size_t(n), C.c_int(1 if on_device else 0),
                                                     C.c_void_p(t.data_ptr()) if t.numel() else None, C.c_size_t(t.numel()), C.byref(got))

        rc = call(out)
        if (rc == _RV_E_ARG or not out.numel()) and got.value > out.numel():  # the capacity answer: the reader has not moved
            out = torch.empty(got.value, dtype=torch.uint8, device=dev)
            rc = call(out)
        _lib.check(rc)
        del keep
        return out.reshape(-1)[:got.value]

    def finish(self):
        """-> (bytes fed, bits delivered) so far"""
        a, b = C.c_uint64(), C.c_uint64()
        _lib.check(_lib.lib().rv_witness_reader_finish(self.handle, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def close(self):
        if self.handle:
            if self.ctx.handle:
                _lib.lib().rv_witness_reader_destroy(self.handle)
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


class DeviceWindows:
    """A GF(2) witness source for the streams (`prove_streaming_pieces`, `evaluate_streaming_pieces`): the witness text `source` -- a
    path (memory-mapped), a buffer or a uint8 GPU tensor -- read in windows of window_bytes on the GPU as the pieces ask for bits.
    `take(n)` returns the next n bits as a uint8 tensor in GPU memory, reading further windows as needed, and raises the library's
    RV_E_WITNESS_SHORT error when the text ends first; `rewind()` starts over (a proof reads the witness once per pass).  It holds at
    most one window of text plus the bits not yet taken."""

    def __init__(self, source, window_bytes: int = 64 << 20, ctx=None):
        from .program_file import _window_source

        self.window_bytes = int(window_bytes)
        if not 0 < self.window_bytes < 1 << 32:
            raise ValueError("window_bytes must be in [1, 2^32)")
        self.ctx = _context(ctx)
        self.data, self.size = _window_source(source)
        self.reader = None
        self.rewind()

    def rewind(self):
        import torch

        if self.reader is not None:
            self.reader.close()
        self.reader = DeviceReader(self.ctx)
        self.at = 0
        self.pending = torch.empty(0, dtype=torch.uint8, device=torch.device("cuda", self.ctx.device))

    def take(self, n: int):
        import torch

        n = int(n)
        parts, have = [self.pending], int(self.pending.numel())
        while have < n and self.at < self.size:
            bits = self.reader.feed(self.data[self.at:self.at + self.window_bytes])
            self.at = min(self.size, self.at + self.window_bytes)
            parts.append(bits)
            have += int(bits.numel())
        if len(parts) > 1:
            self.pending = torch.cat(parts)
        if have < n:
            raise _lib.ReverieError(_RV_E_WITNESS_SHORT, f"the witness text ends after {self.reader.finish()[1]} bits")
        out, self.pending = self.pending[:n], self.pending[n:].clone() if have > n else self.pending[:0]
        return out

    def close(self):
        if self.reader is not None:
            self.reader.close()
            self.reader = None
        self.data = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
