"""The Bristol texts the parser tests share (test_bristol_header_host.py, test_gpu_bristol_device.py): well-formed texts, random
netlists around the device parser's tile sizes, error texts with the code the host parser gives each, and the raw calls of both parsers.

Nothing here needs a GPU but `device_parse`; the texts are built in Python (adder64 and AES-128 come from bristol_gen)."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from reverie_amd import _lib
from reverie_amd.ops import OP_DTYPE

BAD_OP, WIRE_OOB, UNSUPPORTED, ARG = 5, 3, 8, 9


@functools.lru_cache(maxsize=None)
def tiles():
    """(bytes of text per tile workgroup, gate lines per line workgroup) of the device parser"""
    out = (C.c_uint32 * 2)()
    assert _lib.lib().rv_hook_bristol_tiles(out) == 0
    return int(out[0]), int(out[1])


# ---- the two parsers, raw: (return code, n_ops, record bytes or None, info dict) ----
def _info(bi):
    return {k: int(getattr(bi, k)) for k, _ in bi._fields_}


def _exp(expected):
    if expected is None:
        return None, 0
    e = np.ascontiguousarray(np.asarray(expected, dtype=np.uint8))
    keep = e if e.size else np.zeros(1, np.uint8)
    return keep, int(e.size)


def host_parse(text: bytes, expected=None, fmt=0):
    e, ne = _exp(expected)
    ops, n, bi = C.c_void_p(), C.c_size_t(), _lib.BristolInfo()
    rc = _lib.lib().rv_bristol_parse(text, C.c_size_t(len(text)), C.c_int(fmt), e.ctypes.data_as(C.c_void_p) if e is not None else None,
                                     C.c_size_t(ne), C.byref(ops), C.byref(n), C.byref(bi))
    if rc:
        return rc, 0, None, None
    recs = C.string_at(ops, n.value * OP_DTYPE.itemsize)
    _lib.lib().rv_free(ops)
    return 0, int(n.value), recs, _info(bi)


def host_header(text: bytes, fmt=0):
    """(return code, info dict, gates offset) of rv_bristol_header"""
    bi, off = _lib.BristolInfo(), C.c_size_t()
    buf = np.frombuffer(text, np.uint8) if len(text) else np.zeros(1, np.uint8)
    rc = _lib.lib().rv_bristol_header(C.c_void_p(buf.ctypes.data), C.c_size_t(len(text)), C.c_int(fmt), C.byref(bi), C.byref(off))
    return rc, _info(bi), int(off.value)


def device_parse(ctx, text, n_text, on_device, expected=None, fmt=0, d_ops=None, cap=0):
    """rv_bristol_parse_device as it is: text is a host address (a numpy uint8 array) or a device address (an int); d_ops a torch uint8
    tensor or None.  -> (return code, *n_ops, info dict)"""
    e, ne = _exp(expected)
    n, bi = C.c_size_t(12345), _lib.BristolInfo()
    p_text = text.ctypes.data if isinstance(text, np.ndarray) else int(text)
    rc = _lib.lib().rv_bristol_parse_device(ctx.handle, C.c_void_p(p_text), C.c_size_t(n_text), C.c_int(1 if on_device else 0), C.c_int(fmt),
                                            C.c_void_p(e.ctypes.data) if e is not None else None, C.c_size_t(ne),
                                            C.c_void_p(d_ops.data_ptr()) if d_ops is not None else None, C.c_size_t(cap), C.byref(n), C.byref(bi))
    return rc, int(n.value), _info(bi)


# ---- building texts ----
def fashion(n_in, n_out, n_wires, lines, sep=b"\n", end=b"\n"):
    return b"%d %d\n1 %d\n1 %d\n\n" % (len(lines), n_wires, n_in, n_out) + sep.join(lines) + (end if lines else b"")


def old(n_in, n_out, n_wires, lines):
    return b"%d %d\n%d 0 %d\n\n" % (len(lines), n_wires, n_in, n_out) + b"\n".join(lines) + b"\n"


def mand(ins_a, ins_b, outs):
    toks = [len(ins_a) * 2, len(outs)] + list(ins_a) + list(ins_b) + list(outs)
    return b" ".join(b"%d" % t for t in toks) + b" MAND"


def random_lines(n_lines, seed, n_in=8, mand_every=0):
    """(lines, n_wires): an SSA netlist of every kind over n_in inputs; mand_every > 0: every that-many-th line is a two-lane MAND"""
    rng = np.random.default_rng(seed)
    lines, w = [], n_in
    for i in range(n_lines):
        a, b = (int(x) for x in rng.integers(0, w, 2))
        k = int(rng.integers(0, 7))
        if mand_every and i % mand_every == mand_every - 1:
            lines.append(mand([a, b], [b, a], [w, w + 1]))
            w += 2
            continue
        if k <= 1:
            lines.append(b"2 1 %d %d %d %s" % (a, b, w, b"XOR" if k else b"AND"))
        elif k == 2:
            lines.append(b"1 1 %d %d INV" % (a, w))
        elif k == 3:
            lines.append(b"1 1 %d %d NOT" % (a, w))
        elif k == 4:
            lines.append(b"1 1 %d %d EQW" % (a, w))
        elif k == 5:
            lines.append(b"1 1 %d %d EQ" % (a & 1, w))
        else:
            lines.append(mand([a], [b], [w]))
        w += 1
    return lines, w


def random_netlist(n_lines, seed, n_in=8, n_out=2, mand_every=0):
    lines, w = random_lines(n_lines, seed, n_in, mand_every)
    return fashion(n_in, min(n_out, w), w, lines)


def _pad_to(text: bytes, length: int) -> bytes:
    """the text with leading zeros in front of its first gate line's first number, so that it is `length` bytes long"""
    rc, _, off = host_header(text)
    assert rc == 0 and length >= len(text)
    at = off
    while text[at:at + 1] in (b"\n", b" "):
        at += 1
    return text[:at] + b"0" * (length - len(text)) + text[at:]


def of_length(length, seed):
    """a random netlist of exactly `length` bytes"""
    n = max(1, (length - 40) // 16)
    while True:
        t = random_netlist(n, seed)
        if len(t) <= length:
            return _pad_to(t, length)
        n -= max(1, (len(t) - length) // 16)


def line_start_at(offset_in_region, seed, n_lines=40):
    """a netlist in which some gate line's first byte lies `offset_in_region` bytes behind the 16-byte-aligned address at or below the
    start of its gate region (where the device parser's tiles start, for a text at an aligned address)"""
    t = random_netlist(n_lines, seed)
    _, _, off = host_header(t)
    base = off & ~15
    lines_at = [i + 1 for i in range(off, len(t) - 1) if t[i:i + 1] == b"\n"]
    want = base + offset_in_region
    first = [s for s in lines_at if s <= want]
    assert len(first) >= 2, "the netlist is too long for the wanted offset: fewer lines"
    shift = want - first[-1]
    at = off
    while t[at:at + 1] in (b"\n", b" "):
        at += 1
    t = t[:at] + b"0" * shift + t[at:]
    assert t[want - 1:want] == b"\n" and t[want:want + 1] not in (b"\n", b" ")
    return t


def long_mand(n_lanes, n_in=4):
    """a MAND line of n_lanes lanes between two ordinary lines"""
    rng = np.random.default_rng(n_lanes)
    a = [int(x) for x in rng.integers(0, n_in, n_lanes)]
    b = [int(x) for x in rng.integers(0, n_in, n_lanes)]
    w = n_in
    lines = [b"2 1 0 1 %d XOR" % w, mand(a, b, list(range(w + 1, w + 1 + n_lanes))), b"2 1 %d %d %d AND" % (w, w + n_lanes, w + 1 + n_lanes)]
    return fashion(n_in, 1, w + 2 + n_lanes, lines)


def well_formed():
    """[(name, text, fmt)]"""
    tile, _ = tiles()
    every = [b"2 1 0 1 4 XOR", b"2 1 0 4 5 AND", b"1 1 5 6 INV", b"1 1 6 7 NOT", b"1 1 7 8 EQW", b"1 1 0 9 EQ", b"1 1 1 10 EQ",
             mand([0, 1], [2, 3], [11, 12])]
    out = [
        ("fashion", fashion(4, 2, 13, every), 0),
        ("fashion-forced", fashion(4, 2, 13, every), 1),
        ("old", old(4, 2, 13, every), 0),
        ("old-forced", old(4, 2, 13, every), 2),
        # "2 a b" on line 2: Fashion when a third header line follows (its last token a number), old Bristol otherwise
        ("ambiguous-fashion", b"2 7\n2 2 2\n1 1\n2 1 0 1 4 XOR\n2 1 2 3 5 AND\n", 0),
        ("ambiguous-old", b"2 6\n2 2 1\n2 1 0 1 4 XOR\n2 1 2 3 5 AND\n", 0),
        ("zero-gates", b"0 4\n1 4\n1 2\n", 0),
        ("zero-gates-no-newline", b"0 4\n1 4\n1 2", 0),
        ("crlf", fashion(4, 2, 13, every).replace(b"\n", b"\r\n"), 0),
        ("tabs", fashion(4, 2, 13, every).replace(b" ", b"\t"), 0),
        ("blanks", fashion(4, 2, 13, [b"  \t" + l + b" \t " for l in every], sep=b"\n\n \t\r\n\n"), 0),
        ("leading-blank-lines", b"\n \n" + fashion(4, 2, 13, every), 0),
        ("no-final-newline", fashion(4, 2, 13, every, end=b""), 0),
        ("trailing-garbage", fashion(4, 2, 13, every) + b"this is no gate\n9 9 9\n\x00\x0b", 0),
        ("more-lines-than-gates", b"3 13\n1 4\n1 2\n" + b"\n".join(every) + b"\n", 0),
        ("leading-zeros", fashion(4, 2, 13, [b"02 0001 00 01 0004 XOR", b"2 1 0 000000000000000000004 5 AND"]), 0),
    ]
    for n in (1, 2, 3, 64, 65):
        out.append(("mand-%d" % n, long_mand(n), 0))
    t = long_mand(tile // 2)  # three tokens of two bytes and more per lane: longer than two tiles
    assert len(t) > 2 * tile + 64
    out.append(("mand-two-tiles", t, 0))
    return out


def boundary_texts():
    """[(name, text, fmt)]: random netlists around the two tile sizes"""
    tile, wg = tiles()
    out = []
    for n in sorted({1, wg - 1, wg, wg + 1, 2 * wg + 1}):
        out.append(("lines-%d" % n, random_netlist(n, n), 0))
    out.append(("lines-%d-mand" % (2 * wg + 1), random_netlist(2 * wg + 1, 7, mand_every=5), 0))
    for m in (1, 2, 3):
        for d in (-1, 0, 1):
            out.append(("bytes-%dx%+d" % (m, d), of_length(m * tile + d, 100 + 3 * m + d), 0))
    # the gate region's tiles start at the 16-byte-aligned address at or below the region: lengths of the REGION around the tile too
    for m in (1, 2):
        for d in (-1, 0, 1, 2):
            out.append(("start-at-%dx%+d" % (m, d), line_start_at(m * tile + d - 1, 200 + 4 * m + d, n_lines=m * tile // 8), 0))
    return out


GOOD5 = [b"2 1 0 1 4 XOR", b"2 1 0 4 5 AND", b"1 1 5 6 INV", b"2 1 5 6 7 XOR", b"2 1 6 7 8 AND"]
# a bad gate line -> the host parser's code (n_wires is 16 in the texts below)
BAD_LINES = [
    ("three-tokens", b"1 1 XOR", BAD_OP),
    ("count-mismatch", b"2 1 0 1 2 4 XOR", BAD_OP),
    ("xor-three-inputs", b"3 1 0 1 2 4 XOR", BAD_OP),
    ("lower-case-kind", b"2 1 0 1 4 xor", BAD_OP),
    ("numeric-last-token", b"2 1 0 1 4 5", BAD_OP),
    ("eq-2", b"1 1 2 4 EQ", BAD_OP),
    ("mand-nout-0", b"0 0 MAND", BAD_OP),
    ("mand-nout-0-b", b"0 0 1 MAND", BAD_OP),
    ("vt-inside-token", b"2 1 0\x0b1 4 XOR", BAD_OP),
    ("0x-before-big", b"2 1 0x 4294967296 4 XOR", BAD_OP),
    ("digits-then-x", b"2 1 0 99999999999x 4 XOR", BAD_OP),
    ("big-before-1x", b"2 1 4294967296 1x 4 XOR", UNSUPPORTED),
    ("wire-2^32", b"2 1 0 1 4294967296 XOR", UNSUPPORTED),
    ("wire-2^32-1", b"2 1 0 1 4294967295 XOR", WIRE_OOB),
    ("wire-n_wires", b"2 1 0 16 4 XOR", WIRE_OOB),
    ("mand-one-lane-oob", b"4 2 0 1 2 16 4 5 MAND", WIRE_OOB),
    ("eq-out-oob", b"1 1 1 16 EQ", WIRE_OOB),
    ("nul-kind", b"2 1 0 1 4 XOR\x00", BAD_OP),
]


def error_texts():
    """[(name, text, expected_outputs, fmt, the host parser's code)]"""
    out = []
    for name, bad, code in BAD_LINES:
        for where in (0, 2, 4):
            lines = list(GOOD5)
            lines[where] = bad
            out.append(("%s@%d" % (name, where), fashion(4, 2, 16, lines), None, 0, code))
    out += [
        ("short-file", b"6 16\n1 4\n1 2\n" + b"\n".join(GOOD5) + b"\n", None, 0, BAD_OP),
        ("short-file-blank-tail", b"6 16\n1 4\n1 2\n" + b"\n".join(GOOD5) + b"\n \n\t\n", None, 0, BAD_OP),
        ("oob-then-bad-kind", fashion(4, 2, 16, [GOOD5[0], b"2 1 0 16 4 XOR", b"2 1 0 1 4 xor"]), None, 0, WIRE_OOB),
        ("bad-kind-then-oob", fashion(4, 2, 16, [GOOD5[0], b"2 1 0 1 4 xor", b"2 1 0 16 4 XOR"]), None, 0, BAD_OP),
        ("empty", b"", None, 0, BAD_OP),
        ("header-only-line-1", b"3 4\n", None, 0, BAD_OP),
        ("n-expected-wrong", fashion(4, 2, 16, GOOD5), [1, 0, 1], 0, ARG),
        ("inputs-beyond-wires", b"1 4\n1 5\n1 1\n2 1 0 1 2 XOR\n", None, 0, WIRE_OOB),
        ("header-number-2^32", b"1 4294967296\n1 4\n1 1\n2 1 0 1 2 XOR\n", None, 0, UNSUPPORTED),
        ("too-many-gates-for-the-text", b"99 16\n1 4\n1 2\n2 1 0 1 4 XOR\n", None, 0, BAD_OP),
        ("too-many-wires-with-assertions", b"1 4294967295\n1 4\n1 1\n2 1 0 1 4 XOR\n", [1], 0, UNSUPPORTED),
    ]
    # two errors of different codes in different tiles: the earlier line wins whichever workgroup finishes first
    tile, wg = tiles()
    lines, w = random_lines(3 * tile // 12, 5)
    assert len(b"\n".join(lines)) > 2 * tile + 200 and len(lines) > 2 * wg
    for first, second, code in ((b"2 1 0 1 %d XOR" % w, b"2 1 0 1 4 xor", WIRE_OOB), (b"2 1 0 1 4 xor", b"2 1 0 1 %d XOR" % w, BAD_OP)):
        two = list(lines)
        two[3], two[-2] = first, second
        out.append(("two-tiles-%d-first" % code, fashion(8, 2, w, two), None, 0, code))
    return out
