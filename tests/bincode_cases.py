"""The program files (bincode of Vec<CombineOperation>) the reader / writer tests share (test_bincode_device_host.py,
test_gpu_bincode_device.py): programs of every record kind, random mixes of the six record lengths at exact total lengths around the
device reader's tile and scan-block sizes, files with one or two defects, and the raw calls of both readers.

Everything is built with program_file.dumps plus byte surgery; nothing here needs a GPU but `device_parse` / `device_write`.  The
expected answer for a file is always the host reader's (rv_program_from_bincode) on the same bytes."""
from __future__ import annotations

import ctypes as C
import functools
import struct

import numpy as np

from reverie_amd import _lib, program_file
from reverie_amd.ops import B2A, GF2, OP_DTYPE, Z64, SizeHint, largest_wires, program

BAD_OP, UNSUPPORTED, ARG = 5, 8, 9
REC = OP_DTYPE.itemsize
M32 = (1 << 32) - 1


@functools.lru_cache(maxsize=None)
def tiles():
    """(bytes per tile of the walk kernels, counted from data[0]; tiles per block of the composing scan)"""
    out = (C.c_uint32 * 2)()
    assert _lib.lib().rv_hook_bincode_tiles(out) == 0
    return int(out[0]), int(out[1])


# ---- the two readers and the two writers, raw ----
def host_parse(data: bytes):
    """-> (return code, n_ops, record bytes or None)"""
    ops, n = C.c_void_p(), C.c_size_t()
    buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
    rc = _lib.lib().rv_program_from_bincode(buf, C.c_size_t(len(data)), C.byref(ops), C.byref(n))
    if rc:
        return rc, 0, None
    recs = C.string_at(ops, n.value * REC)
    _lib.lib().rv_free(ops)
    return 0, int(n.value), recs


def host_write(recs: bytes):
    """-> (return code, file bytes or None) of rv_program_to_bincode"""
    out, n = C.c_void_p(), C.c_size_t()
    buf = (C.c_uint8 * max(len(recs), 1)).from_buffer_copy(recs or b"\0")
    rc = _lib.lib().rv_program_to_bincode(buf, C.c_size_t(len(recs) // REC), C.byref(out), C.byref(n))
    if rc:
        return rc, None
    data = C.string_at(out, n.value)
    _lib.lib().rv_free(out)
    return 0, data


def expected_info(data: bytes, recs: bytes) -> dict:
    """rv_program_info of a file the host reader accepts, from its records"""
    prog = np.frombuffer(recs, OP_DTYPE)
    z64, gf2 = largest_wires(prog) if len(prog) else (0, 0)
    dom = prog["domain"]
    return {"n_ops": len(prog), "bytes": len(program_file.dumps(prog)), "z64_wires": int(z64), "gf2_wires": int(gf2),
            "n_gf2": int((dom == 0).sum()), "n_z64": int((dom == 1).sum()), "n_b2a": int((dom == 2).sum()), "n_sizehint": int((dom == 3).sum())}


def _info(pi):
    return {k: int(getattr(pi, k)) for k, _ in pi._fields_}


def device_parse(ctx, data, n_data, on_device, d_ops=None, cap=0, null_n=False, null_info=False):
    """rv_program_from_bincode_device as it is: data is a host address (a numpy uint8 array) or a device address (an int); d_ops a
    torch uint8 tensor, a device address or None.  -> (return code, *n_ops, info dict)"""
    n, pi = C.c_size_t(12345), _lib.ProgramInfo()
    p = data.ctypes.data if isinstance(data, np.ndarray) else int(data)
    p_ops = None if d_ops is None else C.c_void_p(d_ops if isinstance(d_ops, int) else d_ops.data_ptr())
    rc = _lib.lib().rv_program_from_bincode_device(ctx.handle, C.c_void_p(p), C.c_size_t(n_data), C.c_int(1 if on_device else 0), p_ops, C.c_size_t(cap),
                                                   None if null_n else C.byref(n), None if null_info else C.byref(pi))
    return rc, int(n.value), _info(pi)


def device_write(ctx, d_ops, n_ops, d_out=None, cap=0):
    """rv_program_to_bincode_device as it is (d_ops / d_out: torch uint8 tensors or None) -> (return code, *len)"""
    n = C.c_size_t(12345)
    rc = _lib.lib().rv_program_to_bincode_device(ctx.handle, C.c_void_p(d_ops.data_ptr()) if d_ops is not None else None, C.c_size_t(n_ops),
                                                 C.c_void_p(d_out.data_ptr()) if d_out is not None else None, C.c_size_t(cap), C.byref(n))
    return rc, int(n.value)


# ---- programs ----
@functools.lru_cache(maxsize=None)
def every_kind():
    """all ten opcodes in both domains, B2A and SizeHint; immediates 0 / 1 and 0, 1, 2^63, 2^64 - 1; wire indices 0 and 2^32 - 1"""
    ops = []
    for D, imms in ((GF2, (0, 1)), (Z64, (0, 1, 1 << 63, (1 << 64) - 1))):
        for w in (0, M32):
            ops += [D.Input(w), D.Random(w), D.Add(w, M32 - w, w), D.Sub(M32 - w, w, w), D.Mul(w, w, M32 - w), D.AssertZero(w)]
            for imm in imms:
                ops += [D.AddConst(w, M32 - w, imm), D.SubConst(M32 - w, w, imm), D.MulConst(w, w, imm), D.Const(w, imm)]
    ops += [B2A(0, M32), B2A(M32, 0), SizeHint(0, M32), SizeHint(M32, 0)]
    return program(ops)


# the ops of each record length (the six lengths of the file format): (domain, opcode, fields)
_BY_LEN = {
    16: [(0, 0, "d"), (0, 1, "d"), (0, 8, "a"), (1, 0, "d"), (1, 8, "a")],
    17: [(0, 9, "d1")],
    20: [(2, 0, "da"), (3, 0, "ab")],
    24: [(1, 9, "d8")],
    25: [(0, 3, "da1"), (0, 5, "da1"), (0, 7, "da1")],
    32: [(0, 2, "dab"), (0, 6, "dab"), (1, 4, "dab"), (1, 3, "da8"), (1, 7, "da8")],
}
LENGTHS = sorted(_BY_LEN)


def ops_of_lengths(lens, rng) -> np.ndarray:
    """a program whose record i takes lens[i] bytes in a file: random kinds of that length, random wires below 2^32, random immediates"""
    lens = np.asarray(lens, dtype=np.int64)
    n = len(lens)
    out = np.zeros(n, OP_DTYPE)
    pick = rng.integers(0, 60, n)
    wires = {f: rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) for f in "dab"}
    imm8, imm1 = rng.integers(0, 1 << 64, n, dtype=np.uint64), rng.integers(0, 2, n).astype(np.uint64)
    for length, kinds in _BY_LEN.items():
        for k, (dom, opc, fields) in enumerate(kinds):
            m = (lens == length) & (pick % len(kinds) == k)
            out["domain"][m], out["opcode"][m] = dom, opc
            for f, name in (("d", "dst"), ("a", "a"), ("b", "b")):
                if f in fields:
                    out[name][m] = wires[f][m]
            if "1" in fields:
                out["imm"][m] = imm1[m]
            if "8" in fields:
                out["imm"][m] = imm8[m]
    assert n == 0 or bool(np.isin(lens, LENGTHS).all())
    return out


def op_of_length(length, rng):
    return tuple(ops_of_lengths([length], rng)[0].tolist())


def fill_16_17(n_bytes, rng) -> np.ndarray:
    """a program of 16- and 17-byte records that takes exactly n_bytes (any n_bytes >= 240, and the smaller sums of 16s and 17s)"""
    y = n_bytes % 16
    x = (n_bytes - 17 * y) // 16
    assert x >= 0 and 16 * x + 17 * y == n_bytes, n_bytes
    lens = np.array([16] * x + [17] * y)
    rng.shuffle(lens)
    return ops_of_lengths(lens, rng)


def mix_of_length(total, seed):
    """a file of exactly `total` bytes (header included): a random mix of all six record lengths"""
    rng = np.random.default_rng(seed)
    assert total - 8 >= 300
    lens = rng.choice(LENGTHS, (total - 8) // 16)
    lens = lens[:int(np.searchsorted(np.cumsum(lens), total - 8 - 300, side="right"))]
    left = total - 8 - int(lens.sum())
    assert 268 <= left <= 332
    data = program_file.dumps(np.concatenate([ops_of_lengths(lens, rng), fill_16_17(left, rng)]))
    assert len(data) == total
    return data


def with_count(data: bytes, count: int) -> bytes:
    return struct.pack("<Q", count) + data[8:]


def count_of(data: bytes) -> int:
    return struct.unpack("<Q", data[:8])[0]


def record_starts(data: bytes):
    """the offsets at which the records of a well-formed file start, by this module's own reading of the tags"""
    n, pos, out = count_of(data), 8, []
    for _ in range(n):
        out.append(pos)
        dom, opc = struct.unpack("<II", data[pos:pos + 8])
        if dom >= 2:
            pos += 20
        else:
            imm = 1 if dom == 0 else 8
            pos += 8 + {0: 8, 1: 8, 2: 24, 3: 16 + imm, 4: 24, 5: 16 + imm, 6: 24, 7: 16 + imm, 8: 8, 9: 8 + imm}[opc]
    return out, pos


def entry_offset_case(e, seed=5):
    """two tiles and a bit: 16- and 17-byte records up to byte T + e - 32, one 32-byte record (so the first record that starts in tile 1
    starts at offset e; e = 0: exactly at T), then a tail"""
    T, _ = tiles()
    rng = np.random.default_rng(seed + e)
    ops = np.concatenate([fill_16_17(T + e - 32 - 8, rng), ops_of_lengths([32, 20, 24, 25, 32, 16, 17, 32, 20], rng)])
    return program_file.dumps(ops)


@functools.lru_cache(maxsize=None)
def boundary_cases():
    """[(name, data)]: total lengths m*T + d and B*T + d, one file across two block boundaries; each with count = the records present,
    one less with a garbage tail behind, one more (RV_E_BAD_OP)"""
    T, B = tiles()
    sizes = [(f"{m}T{d:+d}", m * T + d) for m in (1, 2, 3) for d in (-1, 0, 1)] + [(f"BT{d:+d}", B * T + d) for d in (-1, 0, 1)]
    sizes.append(("2BT+T", 2 * B * T + T + 5))
    out = []
    for k, (name, total) in enumerate(sizes):
        data = mix_of_length(total, 100 + k)
        n = count_of(data)
        out.append((name, data))
        starts, _ = record_starts(data)
        out.append((name + "-count-1-garbage", with_count(data[:starts[-1]], n - 1) + b"\xff" * 40))
        out.append((name + "-count+1", with_count(data, n + 1)))
    return out


# ---- defects ----
def _set(data, at, value: bytes):
    return data[:at] + value + data[at + len(value):]


# name -> (the op the defect needs at the record, what it does to the file given the record's offset)
DEFECTS = {
    "domain": (lambda: GF2.Add(1, 2, 3), lambda d, p: _set(d, p, struct.pack("<I", 4))),
    "opcode": (lambda: Z64.Add(1, 2, 3), lambda d, p: _set(d, p + 4, struct.pack("<I", 10))),
    "imm2-addconst": (lambda: GF2.AddConst(1, 2, 1), lambda d, p: _set(d, p + 24, b"\x02")),
    "imm2-const": (lambda: GF2.Const(1, 1), lambda d, p: _set(d, p + 16, b"\x02")),
    "dst": (lambda: GF2.Add(1, 2, 3), lambda d, p: _set(d, p + 8, struct.pack("<Q", 1 << 32))),
    "a": (lambda: Z64.Add(1, 2, 3), lambda d, p: _set(d, p + 16, struct.pack("<Q", 1 << 32))),
    "b": (lambda: GF2.Mul(1, 2, 3), lambda d, p: _set(d, p + 24, struct.pack("<Q", 1 << 32))),
}
DEFECT_CODE = {"domain": BAD_OP, "opcode": BAD_OP, "imm2-addconst": BAD_OP, "imm2-const": BAD_OP, "dst": UNSUPPORTED, "a": UNSUPPORTED, "b": UNSUPPORTED}


@functools.lru_cache(maxsize=None)
def _random_ops(n_ops, seed):
    rng = np.random.default_rng(seed)
    return ops_of_lengths(rng.choice(LENGTHS, n_ops), rng)


def with_defects(n_ops, defects, seed=9, count=None):
    """a random mix of n_ops records with the defects [(record index, name)] (several may name one record: use ops that carry them
    all, see both_in_one); count: the header's (default n_ops)"""
    ops = _random_ops(n_ops, seed).copy()
    for i, name in defects:
        ops[i] = DEFECTS[name][0]()
    data = program_file.dumps(ops)
    starts, _ = record_starts(data)
    for i, name in defects:
        data = DEFECTS[name][1](data, starts[i])
    return with_count(data, n_ops if count is None else count)


@functools.lru_cache(maxsize=None)
def single_defect_cases():
    """every defect at record 0, in the middle and last"""
    n = 41
    return [(f"{name}@{i}", with_defects(n, [(i, name)], seed=20 + k), DEFECT_CODE[name]) for k, name in enumerate(DEFECTS) for i in (0, n // 2, n - 1)]


@functools.lru_cache(maxsize=None)
def truncation_cases():
    """a file cut after each field of its last record, for every record kind (the tags count as fields); and inside the header"""
    rng = np.random.default_rng(3)
    out = []
    kinds = [GF2.Input(5), GF2.Add(1, 2, 3), GF2.AddConst(1, 2, 1), GF2.AssertZero(7), GF2.Const(3, 1), Z64.Random(5), Z64.Mul(1, 2, 3), Z64.SubConst(1, 2, 9),
             Z64.AssertZero(7), Z64.Const(3, 1 << 40), B2A(1, 2), SizeHint(3, 4)]
    for k, op in enumerate(kinds):
        data = program_file.dumps(program([op_of_length(int(rng.choice(LENGTHS)), rng) for _ in range(3)] + [op]))
        starts, end = record_starts(data)
        last = starts[-1]
        cuts = [last, last + 4] + list(range(last + (8 if op[0] < 2 else 4), end, 8))
        out += [(f"kind{k}-cut{c - last}", data[:c]) for c in sorted(set(cuts)) if c < end]
        out.append((f"kind{k}-cut-1", data[:end - 1]))
    return out


@functools.lru_cache(maxsize=None)
def ordering_cases():
    """[(name, data, expected code or None)]: two defects and which one answers; the pairs again in different tiles and in different
    scan blocks (None: the host reader's answer is all the test needs)"""
    T, B = tiles()
    out = [
        ("unsupported-then-bad", with_defects(30, [(7, "a"), (19, "opcode")]), UNSUPPORTED),
        ("bad-then-unsupported", with_defects(30, [(7, "domain"), (19, "b")]), BAD_OP),
        ("unsupported-then-imm", with_defects(30, [(3, "dst"), (4, "imm2-const")]), UNSUPPORTED),
        ("defect-at-count", with_defects(30, [(20, "opcode")], count=20), 0),
        ("defect-behind-count", with_defects(30, [(25, "dst"), (29, "domain")], count=21), 0),
        ("defect-below-count", with_defects(30, [(19, "dst")], count=20), UNSUPPORTED),
    ]
    # both in one record: an AddConst whose bool is 2 and whose dst is 2^32
    d = with_defects(30, [(11, "imm2-addconst")])
    starts, _ = record_starts(d)
    out.append(("both-in-one-record", _set(d, starts[11] + 8, struct.pack("<Q", 1 << 32)), BAD_OP))
    # a truncated last record whose visible wire bytes are above 2^32 - 1
    d = with_defects(12, [(11, "dst")])
    out.append(("truncated-with-big-wire", d[:-3], BAD_OP))
    # the two defects in different tiles (records of 16 .. 32 bytes: 3 T / 16 records reach the fourth tile) and in different blocks
    per_tile = T // 16
    n = 3 * per_tile
    out.append(("tiles-unsupported-then-bad", with_defects(n, [(10, "b"), (n - 5, "domain")]), UNSUPPORTED))
    out.append(("tiles-bad-then-unsupported", with_defects(n, [(10, "imm2-const"), (n - 5, "a")]), BAD_OP))
    n = (B + 2) * per_tile
    out.append(("blocks-unsupported-then-bad", with_defects(n, [(per_tile, "dst"), (n - 3, "opcode")]), UNSUPPORTED))
    out.append(("blocks-bad-then-unsupported", with_defects(n, [(per_tile, "opcode"), (n - 3, "dst")]), BAD_OP))
    out.append(("blocks-defect-behind-count", with_defects(n, [(n - 3, "opcode")], count=n - 3), 0))
    return out


@functools.lru_cache(maxsize=None)
def header_cases():
    """len 0 .. 7, and counts no file of that length can hold"""
    whole = program_file.dumps(every_kind()[:9])
    out = [(f"len{k}", whole[:k]) for k in range(8)]
    out.append(("count-max", with_count(whole, (1 << 64) - 1)))
    out.append(("count-bound+1", with_count(whole, (len(whole) - 8) // 16 + 1)))
    out.append(("count-bound", with_count(whole, (len(whole) - 8) // 16)))  # (passes the header; too few records)
    return out


@functools.lru_cache(maxsize=None)
def all_files():
    """[(name, data)]: every file above (the corpus of the CPU model and of the device parity test)"""
    out = [("every-kind", program_file.dumps(every_kind())), ("empty", program_file.dumps(program([]))), ("one-record", program_file.dumps(program([Z64.MulConst(1, 2, 3)])))]
    out += [(f"entry{e}", entry_offset_case(e)) for e in range(32)]
    out += boundary_cases()
    out += [(n, d) for n, d, _ in single_defect_cases()] + truncation_cases() + [(n, d) for n, d, _ in ordering_cases()] + header_cases()
    return out
