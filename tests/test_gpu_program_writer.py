"""rv_program_writer_* against rv_program_to_bincode (the host definition): the bytes of all feeds, in order, are the whole file's for
every way of cutting the list; reader o writer in windows is the identity on records; and rv_program_to_bincode_device, whose
kernels the windowed writer now shares, still gives the host writer's bytes and codes on the shared corpus."""
import ctypes as C

import numpy as np
import pytest

import bincode_cases as bc
from reverie_amd import _lib
from reverie_amd.ops import OP_DTYPE

pytestmark = pytest.mark.gpu
REC = OP_DTYPE.itemsize
ARG, BAD_OP, UNSUPPORTED = 9, 5, 8


@pytest.fixture(scope="module")
def ctx():
    import reverie_amd

    return reverie_amd.Context.default()


def to_gpu(program):
    import torch

    return torch.from_numpy(np.frombuffer(program.tobytes() or b"\0" * REC, np.uint8).copy()).cuda()


class Writer:
    def __init__(self, ctx, n_ops):
        self.h = C.c_void_p()
        self.rc = _lib.lib().rv_program_writer_begin(ctx.handle, C.c_uint64(n_ops), C.byref(self.h))

    def feed(self, ops, on_device, cap=None, lead=0):
        """-> (code, piece dict, the bytes written); the buffer begins `lead` bytes into an aligned allocation"""
        import torch

        n = len(ops)
        keep = to_gpu(ops) if on_device else np.ascontiguousarray(ops)
        p = (keep.data_ptr() if on_device else keep.ctypes.data) if n else None
        cap = 8 + 32 * n if cap is None else cap
        buf = torch.full((lead + max(cap, 1) + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        piece = _lib.WriterPiece()
        rc = _lib.lib().rv_program_writer_feed(self.h, C.c_void_p(p) if p else None, C.c_size_t(n), C.c_int(1 if on_device else 0),
                                               C.c_void_p(buf.data_ptr() + lead), C.c_size_t(cap), C.byref(piece))
        torch.cuda.synchronize()
        out = buf.cpu().numpy().tobytes()
        d = {k: int(getattr(piece, k)) for k, _ in piece._fields_}
        if rc:
            assert out == b"\xA5" * len(out), "a refused feed wrote something"
            return rc, d, b""
        assert out[:lead] == b"\xA5" * lead and out[lead + d["bytes"]:] == b"\xA5" * (len(out) - lead - d["bytes"]), "bytes around the piece were written"
        return rc, d, out[lead:lead + d["bytes"]]

    def finish(self):
        return _lib.lib().rv_program_writer_finish(self.h)

    def close(self):
        _lib.lib().rv_program_writer_destroy(self.h)


def six_lengths(n, seed):
    """n records whose lengths cycle through the six of the file format, so that each lies on both sides of any cut in the middle"""
    return bc.ops_of_lengths([bc.LENGTHS[(i * 5 + i // 6) % 6] for i in range(n)], np.random.default_rng(seed))


def test_every_pair_of_cuts(ctx):
    p = six_lengths(40, 3)
    rc, data = bc.host_write(p.tobytes())
    assert rc == 0
    for at in (13, 20, 27):  # each length on both sides of a cut
        assert {len(bc.host_write(p[i:i + 1].tobytes())[1]) - 8 for i in range(at)} == set(bc.LENGTHS)
        assert {len(bc.host_write(p[i:i + 1].tobytes())[1]) - 8 for i in range(at, 40)} == set(bc.LENGTHS)
    n, k = len(p), 0
    for c1 in range(n + 1):
        for c2 in range(c1, n + 1):
            w = Writer(ctx, n)
            assert w.rc == 0 and w.finish() == ARG
            got = b""
            for f, (lo, hi) in enumerate(((0, c1), (c1, c2), (c2, n))):
                rc, piece, part = w.feed(p[lo:hi], on_device=(k + f) % 2 == 0, lead=(k + 5 * f) % 16)
                assert rc == 0 and piece == {"first_op": lo, "n_ops": hi - lo, "file_off": len(got), "bytes": len(part)}
                got += part
                assert w.finish() == (0 if hi == n else ARG)
            assert got == data
            w.close()
            k += 1


def test_cuts_around_the_workgroup(ctx):
    p = six_lengths(2 * 256 + 3, 4)
    rc, data = bc.host_write(p.tobytes())
    for cuts in ((255, 257), (256, 512), (1, 257), (0, 514)):
        w = Writer(ctx, len(p))
        got = b""
        for lo, hi in zip((0,) + cuts, cuts + (len(p),)):
            rc, piece, part = w.feed(p[lo:hi], on_device=lo != 0, lead=lo % 16)
            assert rc == 0 and piece["file_off"] == len(got)
            got += part
        assert got == data and w.finish() == 0
        w.close()


def test_capacity_errors_and_counts(ctx):
    p = six_lengths(30, 5)
    rc, data = bc.host_write(p.tobytes())
    w = Writer(ctx, len(p))
    rc, piece, head = w.feed(p[:0], True, cap=7)  # the header alone does not fit
    assert rc == ARG and piece["bytes"] == 8
    rc, piece, first = w.feed(p[:11], True)
    assert rc == 0 and first == data[:len(first)]
    need = len(data) - len(first)
    rc, piece, _ = w.feed(p[11:], False, cap=need - 1)
    assert rc == ARG and piece == {"first_op": 11, "n_ops": 19, "file_off": len(first), "bytes": need} and w.finish() == ARG
    rc, piece, rest = w.feed(p[11:], True, cap=need)
    assert rc == 0 and first + rest == data and w.finish() == 0
    assert w.feed(p[:1], True)[0] == ARG and w.finish() == 0  # past n_ops
    w.close()
    # a bad record: the host writer's code; then only destroy
    q = p.copy()
    q["reserved"][17] = 1
    assert bc.host_write(q.tobytes())[0] == BAD_OP
    w = Writer(ctx, len(q))
    assert w.feed(q[:17], True)[0] == 0 and w.feed(q[17:20], False)[0] == BAD_OP
    assert w.feed(q[20:], True)[0] == ARG and w.finish() == ARG
    w.close()
    # counts of 2^32 and more go into the header as they are; an empty list is a header
    w = Writer(ctx, (1 << 32) + 5)
    rc, piece, head = w.feed(p[:0], True)
    assert rc == 0 and head == ((1 << 32) + 5).to_bytes(8, "little") and w.finish() == ARG
    w.close()
    w = Writer(ctx, 0)
    assert w.finish() == ARG and w.feed(p[:0], False)[2] == bytes(8) and w.finish() == 0
    w.close()


def test_reader_of_writer_in_windows_is_the_identity(ctx):
    from reverie_amd import program_file

    p = six_lengths(3000, 6)
    parts = []
    with program_file.DeviceWriter(len(p)) as w:
        for lo in range(0, len(p), 700):
            ops = p[lo:lo + 700]
            data, piece = w.feed(to_gpu(ops).reshape(-1, REC) if lo % 1400 else ops)
            assert piece["first_op"] == lo and piece["n_ops"] == len(ops)
            parts.append(data)
        w.finish()
    import torch

    data = torch.cat(parts)
    assert data.cpu().numpy().tobytes() == program_file.dumps(p)
    for window in (1000, 4096 + 17, 50000):
        back = [ops.cpu().numpy().tobytes() for ops, _ in program_file.iter_device(data, window)]
        assert b"".join(back) == p.tobytes()


def test_write_device_to_a_file(ctx, tmp_path):
    from reverie_amd import program_file

    p = six_lengths(1000, 7)
    path = str(tmp_path / "out.bin")
    pieces = ((to_gpu(p[lo:lo + 301]).reshape(-1, REC), None) for lo in range(0, len(p), 301))
    assert program_file.write_device(pieces, path, len(p)) == len(program_file.dumps(p))
    assert open(path, "rb").read() == program_file.dumps(p)


def test_whole_list_writer_still_equals_the_host_writer(ctx):
    """rv_program_to_bincode_device on the shared corpus' lists: bytes, codes, the sizing call and the short buffer"""
    import torch

    lists = [np.frombuffer(bc.host_parse(data)[2], OP_DTYPE) for name, data in bc.all_files() if bc.host_parse(data)[0] == 0]
    bad = six_lengths(600, 8)
    bad["domain"][300] = 7
    assert len(lists) >= 10
    for p in lists + [six_lengths(0, 1), six_lengths(257, 2), bad]:
        rc, data = bc.host_write(p.tobytes())
        d_ops = to_gpu(p) if len(p) else None
        got_rc, n = bc.device_write(ctx, d_ops, len(p))
        assert (got_rc, n) == ((rc, 0) if rc else (ARG, len(data)))
        if rc:
            continue
        for lead in (0, 5):
            buf = torch.full((lead + len(data) + 16,), 0xA5, dtype=torch.uint8, device="cuda")
            assert bc.device_write(ctx, d_ops, len(p), buf[lead:], len(data)) == (0, len(data))
            out = buf.cpu().numpy().tobytes()
            assert out[lead:lead + len(data)] == data and out[:lead] + out[lead + len(data):] == b"\xA5" * (lead + 16)
        buf = torch.full((len(data),), 0xA5, dtype=torch.uint8, device="cuda")
        assert bc.device_write(ctx, d_ops, len(p), buf, len(data) - 1) == (ARG, len(data))
        assert buf.cpu().numpy().tobytes() == b"\xA5" * len(data)
