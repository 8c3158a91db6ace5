"""rv_bristol_write_device and rv_bristol_writer_* against rv_bristol_write (the host definition, itself pinned to `bristol.dumps` by
tests/test_bristol_write_host.py): device bytes == host bytes throughout, the same code for every record list, sizes around the emit
tile and the scan block, d_text at every alignment with guard bytes, the capacity protocol, and the windowed writer for every cut."""
import ctypes as C

import numpy as np
import pytest

import bristol_write_cases as bw
from reverie_amd import _lib
from reverie_amd.ops import OP_DTYPE

pytestmark = pytest.mark.gpu
REC = OP_DTYPE.itemsize
GUARD = 64


@pytest.fixture(scope="module")
def ctx():
    import reverie_amd

    return reverie_amd.Context.default()


@pytest.fixture(scope="module")
def tiles():
    out = (C.c_uint32 * 2)()
    assert _lib.lib().rv_hook_bristol_write_tiles(out) == 0
    return int(out[0]), int(out[1])


def host_write(program, n_outputs=0, n_wires=None):
    """-> (code, text): rv_bristol_write"""
    L = _lib.lib()
    p = np.ascontiguousarray(program)
    out, n = C.c_void_p(), C.c_size_t()
    rc = L.rv_bristol_write(C.c_void_p(p.ctypes.data) if len(p) else None, C.c_size_t(len(p)), C.c_uint64(n_wires or 0), C.c_uint64(n_outputs),
                            C.byref(out), C.byref(n))
    text = C.string_at(out, n.value) if rc == 0 else None
    if out:
        L.rv_free(out)
    return rc, text


def to_gpu(program):
    import torch

    return torch.from_numpy(np.frombuffer(program.tobytes() or b"\0" * REC, np.uint8).copy()).cuda()


def device_write(ctx, d_ops, n_ops, n_outputs, n_wires, buf, offset, cap):
    """-> (code, *len): rv_bristol_write_device into buf[offset, offset + cap) (buf None: a sizing call)"""
    import torch

    n = C.c_size_t(12345)
    rc = _lib.lib().rv_bristol_write_device(ctx.handle, C.c_void_p(d_ops.data_ptr()) if n_ops else None, C.c_size_t(n_ops), C.c_uint64(n_wires or 0),
                                            C.c_uint64(n_outputs), C.c_void_p(buf.data_ptr() + offset) if buf is not None else None, C.c_size_t(cap),
                                            C.byref(n))
    torch.cuda.synchronize()
    return rc, int(n.value)


def check(ctx, program, n_outputs=0, n_wires=None, offsets=(0,)):
    """the device writer's answer is the host writer's: the code; the bytes at each offset of d_text from an aligned allocation, with
    the guard bytes before and behind untouched; cap = len - 1 and the sizing call"""
    import torch

    rc, text = host_write(program, n_outputs, n_wires)
    d_ops = to_gpu(program)
    size = len(text) if text is not None else 41 * len(program) + 96
    for off in offsets:
        buf = torch.full((GUARD + 16 + size + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        got = device_write(ctx, d_ops, len(program), n_outputs, n_wires, buf, GUARD + off, size)
        out = buf.cpu().numpy().tobytes()
        if rc:
            assert got == (rc, 0), (got, rc)
            assert out == b"\xA5" * len(out), "a list with a code wrote something"
        else:
            assert got == (0, len(text)), (got, len(text), off)
            assert out[GUARD + off:GUARD + off + size] == text, off
            assert out[:GUARD + off] == b"\xA5" * (GUARD + off) and out[GUARD + off + size:] == b"\xA5" * (16 - off + GUARD), off
    # a sizing call: the records' own code, or RV_E_ARG and the length
    assert device_write(ctx, d_ops, len(program), n_outputs, n_wires, None, 0, 0) == ((rc, 0) if rc else (bw.ARG, len(text)))
    if rc == 0:  # one byte short: RV_E_ARG, the length, nothing written
        buf = torch.full((len(text) + 16,), 0x5A, dtype=torch.uint8, device="cuda")
        assert device_write(ctx, d_ops, len(program), n_outputs, n_wires, buf, 0, len(text) - 1) == (bw.ARG, len(text))
        assert buf.cpu().numpy().tobytes() == b"\x5A" * (len(text) + 16)
    return rc, text


@pytest.mark.parametrize("name,program,n_outputs,n_wires", bw.ok_cases(), ids=[c[0] for c in bw.ok_cases()])
def test_bytes_are_the_host_bytes(ctx, name, program, n_outputs, n_wires):
    rc, text = check(ctx, program, n_outputs, n_wires)
    assert rc == 0 and text == bw.expect(program, n_outputs, n_wires)


@pytest.mark.parametrize("name,program,n_outputs,n_wires,code", bw.bad_cases(), ids=[c[0] for c in bw.bad_cases()])
def test_codes_are_the_host_codes(ctx, name, program, n_outputs, n_wires, code):
    assert check(ctx, program, n_outputs, n_wires) == (code, None)


def test_sizes_around_the_tile_and_the_scan_block(ctx, tiles):
    T, S = tiles
    for n in sorted({T - 1, T, T + 1, 2 * T + 1, S - 1, S, S + 1}):
        rc, text = check(ctx, bw.random_program(3, n - 3, n), 1)
        assert rc == 0 and text.count(b"\n") == 4 + n - 3
        rc, text = check(ctx, bw.random_program(0, n, n + 1, junk=True))
        assert rc == 0
    # inputs that fill a workgroup, and more: workgroups without a byte of their own
    assert check(ctx, bw.prog(bw.inputs(2 * T + 5) + [bw.XOR(2 * T + 5, 0, 2 * T + 4)]), 3)[0] == 0
    assert check(ctx, bw.prog(bw.inputs(T)))[0] == 0


def test_shortest_and_longest_lines_at_a_workgroups_ends(ctx, tiles):
    """where a neighbour's bytes share a 16-byte chunk: every pairing of the two line lengths across the boundaries of three tiles"""
    T, _ = tiles
    for left in (bw.SHORTEST, bw.LONGEST):
        for right in (bw.SHORTEST, bw.LONGEST):
            for fill in (bw.SHORTEST, bw.LONGEST, bw.INV(12345, 678)):
                tile = [right] + [fill] * (T - 2) + [left]
                assert check(ctx, bw.prog(tile * 3 + [right]))[0] == 0


def test_every_alignment_of_the_text(ctx, tiles):
    T, _ = tiles
    for program in (bw.random_program(3, 2 * T + 9, 77), bw.prog([bw.SHORTEST]), bw.prog([]), bw.digit_boundary_program()):
        assert check(ctx, program, 0, None, offsets=range(16))[0] == 0


def test_bad_records_by_position(ctx, tiles):
    T, _ = tiles
    n = 3 * T + 7
    good = bw.random_program(4, n - 4, 5)
    bad_op, unsup = bw.prog([bw.op(bw.ADD, 9, 0, 1, reserved=1)])[0], bw.prog([bw.op(bw.SUB, 9, 0, 1)])[0]
    for where in (4, n - 1, T - 1, T, 2 * T):
        p = good.copy()
        p[where] = unsup
        assert check(ctx, p) == (bw.UNSUPPORTED, None)
    # the first record of all: an Input that is out of place
    p = good.copy()
    p["dst"][0] = 1
    assert check(ctx, p) == (bw.UNSUPPORTED, None)
    # two bad records in different workgroups: the first in list order wins, whichever it is
    for first, second, code in ((unsup, bad_op, bw.UNSUPPORTED), (bad_op, unsup, bw.BAD_OP)):
        p = good.copy()
        p[T + 3], p[2 * T + 11] = first, second
        assert check(ctx, p) == (code, None)
    # ... and a stated wire count that one index in the last workgroup reaches
    p = good.copy()
    p["dst"][n - 2] = n + 50
    assert check(ctx, p, 0, n + 50) == (bw.WIRE_OOB, None)
    assert check(ctx, p, 0, n + 51)[0] == 0


def test_argument_errors(ctx):
    import torch

    L = _lib.lib()
    p = bw.random_program(2, 6, 1)
    d_ops = to_gpu(p)
    buf = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    n = C.c_size_t()
    a = (C.c_uint64(0), C.c_uint64(0), C.c_void_p(buf.data_ptr()), C.c_size_t(1024))
    assert L.rv_bristol_write_device(None, C.c_void_p(d_ops.data_ptr()), C.c_size_t(len(p)), *a, C.byref(n)) == bw.ARG
    assert L.rv_bristol_write_device(ctx.handle, None, C.c_size_t(len(p)), *a, C.byref(n)) == bw.ARG
    assert L.rv_bristol_write_device(ctx.handle, C.c_void_p(d_ops.data_ptr()), C.c_size_t(len(p)), *a, None) == bw.ARG
    assert L.rv_bristol_write_device(ctx.handle, C.c_void_p(d_ops.data_ptr() + 4), C.c_size_t(len(p) - 1), *a, C.byref(n)) == bw.ARG  # misaligned ops
    assert L.rv_bristol_write_device(ctx.handle, C.c_void_p(p.ctypes.data), C.c_size_t(len(p)), *a, C.byref(n)) == bw.ARG  # host memory


def test_python_dumps_device(ctx):
    from reverie_amd import bristol

    p = bw.random_program(5, 700, 9)
    text = bristol.dumps_device(to_gpu(p).reshape(-1, REC), 2)
    assert text.is_cuda and text.cpu().numpy().tobytes() == bristol.dumps(p, 2)
    back, info = bristol.parse_device(text)
    assert back.cpu().numpy().tobytes() == p.tobytes() and info["n_outputs"] == 2
    with pytest.raises(_lib.ReverieError) as e:
        bristol.dumps_device(to_gpu(bw.bad_cases()[6][1]).reshape(-1, REC))
    assert e.value.code == bw.UNSUPPORTED


# ---- the windowed writer ----
class Writer:
    def __init__(self, ctx, n_ops, n_inputs, n_wires, n_outputs=0):
        self.h = C.c_void_p()
        self.rc = _lib.lib().rv_bristol_writer_begin(ctx.handle, C.c_uint64(n_ops), C.c_uint64(n_inputs), C.c_uint64(n_wires), C.c_uint64(n_outputs),
                                                     C.byref(self.h))

    def feed(self, ops, on_device, cap=None, buf=None):
        """-> (code, piece dict, the bytes written)"""
        import torch

        n = len(ops)
        keep = to_gpu(ops) if on_device else np.ascontiguousarray(ops)
        p = (keep.data_ptr() if on_device else keep.ctypes.data) if n else None
        cap = 96 + 41 * n if cap is None else cap
        buf = torch.full((max(cap, 1) + 16,), 0xA5, dtype=torch.uint8, device="cuda") if buf is None else buf
        piece = _lib.WriterPiece()
        rc = _lib.lib().rv_bristol_writer_feed(self.h, C.c_void_p(p) if p else None, C.c_size_t(n), C.c_int(1 if on_device else 0),
                                               C.c_void_p(buf.data_ptr()), C.c_size_t(cap), C.byref(piece))
        torch.cuda.synchronize()
        out = buf.cpu().numpy().tobytes()
        d = {k: int(getattr(piece, k)) for k, _ in piece._fields_}
        if rc == 0:
            assert out[d["bytes"]:] == b"\xA5" * (len(out) - d["bytes"]), "bytes behind the piece were written"
            return rc, d, out[:d["bytes"]]
        if rc == bw.ARG:
            assert out == b"\xA5" * len(out), "a refused feed wrote something"
        return rc, d, b""

    def finish(self):
        return _lib.lib().rv_bristol_writer_finish(self.h)

    def close(self):
        _lib.lib().rv_bristol_writer_destroy(self.h)


def test_writer_every_pair_of_cuts(ctx):
    p = bw.random_program(5, 36, 21, junk=True)
    rc, text = host_write(p, 3)
    n_in, n_wires = bw.derived(p)
    assert rc == 0 and n_in == 5
    n, k = len(p), 0
    for c1 in range(n + 1):
        for c2 in range(c1, n + 1):
            w = Writer(ctx, n, n_in, n_wires, 3)
            assert w.rc == 0 and w.finish() == bw.ARG
            got, at = b"", 0
            for f, (lo, hi) in enumerate(((0, c1), (c1, c2), (c2, n))):
                rc, piece, data = w.feed(p[lo:hi], on_device=(k + f) % 2 == 0)
                assert rc == 0 and piece == {"first_op": lo, "n_ops": hi - lo, "file_off": at, "bytes": len(data)}
                got, at = got + data, at + len(data)
                assert w.finish() == (0 if hi == n else bw.ARG)
            assert got == text and w.finish() == 0
            w.close()
            k += 1


def test_writer_cuts_around_the_tile(ctx, tiles):
    T, _ = tiles
    p = bw.random_program(7, 2 * T + 3 - 7, 31)
    rc, text = host_write(p, 1)
    n_in, n_wires = bw.derived(p)
    for cuts in ((T - 1, T + 1), (T, 2 * T), (1, T + 1), (T - 1, 2 * T + 2)):
        w = Writer(ctx, len(p), n_in, n_wires, 1)
        got = b""
        for lo, hi in zip((0,) + cuts, cuts + (len(p),)):
            rc, piece, data = w.feed(p[lo:hi], on_device=lo != 0)
            assert rc == 0 and piece["file_off"] == len(got)
            got += data
        assert got == text and w.finish() == 0
        w.close()


def test_writer_capacity_answer_leaves_it_unchanged(ctx):
    p = bw.random_program(2, 30, 41)
    rc, text = host_write(p)
    n_in, n_wires = bw.derived(p)
    w = Writer(ctx, len(p), n_in, n_wires)
    rc, piece, data = w.feed(p[:20], True)
    assert rc == 0
    need = len(text) - len(data)
    rc, piece, _ = w.feed(p[20:], True, cap=need - 1)
    assert rc == bw.ARG and piece == {"first_op": 20, "n_ops": len(p) - 20, "file_off": len(data), "bytes": need}
    assert w.finish() == bw.ARG
    rc, piece2, more = w.feed(p[20:], False, cap=need)
    assert rc == 0 and piece2 == piece and data + more == text and w.finish() == 0
    # past n_ops: refused, nothing moves
    assert w.feed(p[:1], True)[0] == bw.ARG and w.finish() == 0
    w.close()
    # the header alone does not fit: the first feed is unchanged too
    w = Writer(ctx, len(p), n_in, n_wires)
    rc, piece, _ = w.feed(p[:0], True, cap=3)
    assert rc == bw.ARG and piece["bytes"] == len(text.split(b"\n\n")[0]) + 2
    rc, piece, head = w.feed(p[:0], True)
    assert rc == 0 and text.startswith(head) and head.endswith(b"\n\n")
    w.close()


def test_writer_errors(ctx):
    p = bw.random_program(3, 20, 51)
    n_in, n_wires = bw.derived(p)
    # after a record's code only destroy is accepted
    q = p.copy()
    q["opcode"][10] = bw.SUB
    w = Writer(ctx, len(q), n_in, n_wires)
    assert w.feed(q[:8], True)[0] == 0
    assert w.feed(q[8:12], False)[0] == bw.UNSUPPORTED
    assert w.feed(q[12:], True)[0] == bw.ARG and w.feed(q[8:8], True)[0] == bw.ARG and w.finish() == bw.ARG
    w.close()
    # what the writer is told at begin is checked record by record
    for n_inputs, lo, code in ((4, 0, bw.UNSUPPORTED), (2, 0, bw.UNSUPPORTED), (3, 0, 0)):
        w = Writer(ctx, len(p), n_inputs, n_wires)
        assert w.feed(p, True)[0] == code
        w.close()
    w = Writer(ctx, len(p), n_in, n_wires - 1)
    assert w.feed(p[:-1], True)[0] == 0 and w.feed(p[-1:], True)[0] == bw.WIRE_OOB
    w.close()
    # the pairs of defects of the whole-list rule, cut in the middle: the first code a feed returns is the list's
    for name, q, n_outputs, wires, code in bw.bad_cases():
        n_inputs = 0
        while n_inputs < len(q) and q[n_inputs]["domain"] == 0 and q[n_inputs]["opcode"] == 0:
            n_inputs += 1
        if wires is None:  # what the whole-list call would derive; for a list with a bad record, a count no index reaches
            wires = bw.derived(q)[1] if bw.want(q) is not None else 1 << 32
        w = Writer(ctx, len(q), n_inputs, wires, n_outputs)
        got = w.rc
        for part in (q[:len(q) // 2], q[len(q) // 2:]):
            got = got or w.feed(part, True)[0]
        assert got == code, name
        if w.h:
            w.close()
    # begin
    assert Writer(ctx, 5, 6, 9).rc == bw.ARG and Writer(ctx, 5, 0, 0).rc == bw.ARG
    assert Writer(ctx, 5, 3, 2).rc == bw.WIRE_OOB and Writer(ctx, 5, 1, 2, 3).rc == bw.WIRE_OOB
    w = Writer(ctx, 0, 0, 0)
    assert w.rc == 0 and w.finish() == bw.ARG
    assert w.feed(p[:0], True)[2] == b"0 0\n1 0\n1 0\n\n" and w.finish() == 0
    w.close()


def test_writer_counts_above_2_32(ctx):
    w = Writer(ctx, (1 << 32) + 5, 2, (1 << 32) + 9, 1)
    rc, piece, head = w.feed(bw.prog([]), True)
    assert rc == 0 and head == b"%d %d\n1 2\n1 1\n\n" % ((1 << 32) + 3, (1 << 32) + 9)
    assert piece == {"first_op": 0, "n_ops": 0, "file_off": 0, "bytes": len(head)} and w.finish() == bw.ARG
    w.close()


def test_python_device_writer_and_write_device(ctx, tmp_path):
    from reverie_amd import bristol

    p = bw.random_program(4, 900, 61)
    n_in, n_wires = bw.derived(p)
    with bristol.DeviceWriter(len(p), n_in, n_wires, 2) as w:
        parts = []
        for lo in range(0, len(p), 250):
            ops = p[lo:lo + 250]
            text, piece = w.feed(to_gpu(ops).reshape(-1, REC) if lo % 500 else ops)
            assert piece["first_op"] == lo and piece["file_off"] == sum(len(x) for x in parts)
            parts.append(text.cpu().numpy().tobytes())
        w.finish()
    assert b"".join(parts) == bristol.dumps(p, 2)
    path = str(tmp_path / "out.txt")
    pieces = ((to_gpu(p[lo:lo + 333]).reshape(-1, REC), {"n": lo}) for lo in range(0, len(p), 333))
    assert bristol.write_device(pieces, path, len(p), n_in, n_wires, 2) == len(bristol.dumps(p, 2))
    assert open(path, "rb").read() == bristol.dumps(p, 2)
