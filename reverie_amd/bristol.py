"""Bristol / Bristol Fashion front end: text -> rv_op program, on the host (`parse`) or on the GPU (`parse_device`).

The reference README advertises Bristol-format circuits but leaves parsing to the
un-vendored `mcircuit` crate (/root/reference/README.md:14-16, src/lib.rs:6-7).  The
parser itself is C++ behind the C-ABI (`rv_bristol_parse`, reverie_amd/csrc/bristol.cpp) and, for a program that is to be made in
GPU memory, kernels behind it (`rv_bristol_parse_device`, reverie_amd/csrc/bristol_dev.hip: DESIGN §18); this is the ctypes wrapper.
`dumps` writes a GF(2) program of Bristol shape back as Fashion text.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .ops import OP_DTYPE


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
