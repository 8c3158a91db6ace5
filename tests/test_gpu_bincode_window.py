"""rv_program_reader_* (a program file read in windows on the GPU) against rv_program_from_bincode on the whole file: for every way
of cutting, the records of all feeds are the host's records, every feed's piece is the defined one (the records whose last byte
has been fed), the first nonzero code is the host's, and no byte behind a window is read -- the windows are slices of one GPU
tensor that holds the whole file, so the bytes right behind a window read as the next records.  Then the Python layers
(program_file.DeviceReader / iter_device / scan_device, stream.*_streaming_pieces) and the command line's --stream."""
import bisect
import ctypes as C
import functools
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import bincode_cases as bc
from conftest import GOLDEN, ROOT, golden_ops
from reverie_amd import _lib
from reverie_amd.ops import OP_DTYPE, program

pytestmark = pytest.mark.gpu
REC = OP_DTYPE.itemsize
FILL = 0xA5
SOURCES = ["host", 0, 1, 2, 3]  # host bytes, or a GPU tensor with the file at this lead


@pytest.fixture(scope="module")
def rv():
    import reverie_amd

    return reverie_amd


@pytest.fixture(scope="module")
def ctx(rv):
    return rv.Context.default()


class Raw:
    """the C calls as they are"""

    def __init__(self, ctx, file_len):
        self.h = C.c_void_p()
        assert _lib.lib().rv_program_reader_begin(ctx.handle, C.c_uint64(file_len), C.byref(self.h)) == 0

    def feed(self, addr, n, on_dev, d_ops=None, cap=0, null_piece=False):
        piece = _lib.ProgramPiece()
        rc = _lib.lib().rv_program_reader_feed(self.h, C.c_void_p(addr), C.c_size_t(n), C.c_int(1 if on_dev else 0),
                                               C.c_void_p(d_ops.data_ptr()) if d_ops is not None else None, C.c_size_t(cap),
                                               None if null_piece else C.byref(piece))
        return rc, {k: int(getattr(piece, k)) for k, _ in piece._fields_}

    def finish(self):
        info = _lib.ProgramInfo()
        rc = _lib.lib().rv_program_reader_finish(self.h, C.byref(info))
        return rc, {k: int(getattr(info, k)) for k, _ in info._fields_}

    def resume(self, file_off, next_op):
        return _lib.lib().rv_hook_program_reader_resume(self.h, C.c_uint64(file_off), C.c_uint64(next_op))

    def close(self):
        if self.h:
            _lib.lib().rv_program_reader_destroy(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Source:
    """the file's bytes for the feeds: host memory, or one GPU tensor (`lead` bytes, the whole file, then more records)"""

    def __init__(self, data: bytes, kind):
        import torch

        self.on_dev = kind != "host"
        if self.on_dev:
            self.keep = torch.from_numpy(np.frombuffer(b"\xee" * kind + data + b"\x00\x00\x00\x00\x02\x00\x00\x00" * 6, np.uint8).copy()).cuda()
            self.base = self.keep.data_ptr() + kind
        else:
            self.keep = np.frombuffer(data + b"\0", np.uint8).copy()
            self.base = self.keep.ctypes.data


@functools.lru_cache(maxsize=6)
def source(data: bytes, kind):
    return Source(data, kind)


@functools.lru_cache(maxsize=4)
def answer(data: bytes):
    """the host reader's (code, count, records), and for a file it accepts its info, the offsets behind its records and its Input
    counts: computed once per file"""
    rc, n, want = bc.host_parse(data)
    if rc:
        return rc, n, want, None, None, None
    prog = np.frombuffer(want, OP_DTYPE)
    starts, end = bc.record_starts(data)
    inputs = tuple(int(((prog["domain"] == d) & (prog["opcode"] == 0)).sum()) for d in (0, 1))
    return rc, n, want, bc.expected_info(data, want), (starts[1:] + [end] if starts else []), inputs


def feed_all(ctx, data, windows, kind, scan=()):
    """the windows (lengths) fed in order -> (first nonzero code, the records of all feeds, the pieces, the reader's finish)"""
    import torch

    src = source(data, kind)
    recs, pieces, at = b"", [], 0
    with Raw(ctx, len(data)) as r:
        for k, w in enumerate(windows):
            cap = w // 16 + 1
            d_ops = None if k in scan else torch.full((cap + 2, REC), FILL, dtype=torch.uint8, device="cuda")
            rc, piece = r.feed(src.base + at, w, src.on_dev, d_ops, cap if d_ops is not None else 0)
            at += w
            if rc:
                # after a code the reader takes nothing more
                assert r.feed(src.base, 0, src.on_dev)[0] == bc.ARG and r.finish()[0] == bc.ARG
                return rc, recs, pieces, None
            assert piece["n_ops"] <= cap
            if d_ops is not None:
                out = d_ops.cpu().numpy().tobytes()
                recs += out[:piece["n_ops"] * REC]
                assert out[piece["n_ops"] * REC:] == bytes([FILL]) * ((cap + 2 - piece["n_ops"]) * REC), "records behind n_ops were written"
            pieces.append(piece)
        return 0, recs, pieces, r.finish()


def ends_of(data):
    starts, end = bc.record_starts(data)
    return starts[1:] + [end] if starts else []


def check(ctx, data, windows, kind):
    """the windows cover the file: the host reader's answer, piece by piece"""
    assert sum(windows) == len(data)
    rc, n, want, info, ends, inputs = answer(data)
    got_rc, recs, pieces, fin = feed_all(ctx, data, windows, kind)
    assert got_rc == rc, (got_rc, rc, windows[:4], kind)
    if rc:
        return
    assert recs == want
    at = done = 0
    for w, piece in zip(windows, pieces):
        at += w
        upto = bisect.bisect_right(ends, at)
        assert (piece["first_op"], piece["n_ops"]) == (done, upto - done), (windows[:4], kind, at)
        done = upto
    assert (sum(p["n_input_gf2"] for p in pieces), sum(p["n_input_z64"] for p in pieces)) == inputs
    assert fin == (0, info)


def fixed(n, w):
    return [min(w, n - at) for at in range(0, n, w)] or [0]


# ---- every cut ----
@pytest.mark.parametrize("kind", SOURCES)
def test_every_cut(ctx, kind):
    """every_kind (all six record lengths) cut at every position into two windows"""
    data = bc.program_file.dumps(bc.every_kind())
    assert answer(data)[0] == 0
    for c in range(len(data) + 1):
        check(ctx, data, [c, len(data) - c], kind)


@pytest.mark.parametrize("kind", SOURCES)
def test_small_windows(ctx, kind):
    """1 and 7 bytes at a time: the header is cut as well, and every record straddles"""
    data = bc.program_file.dumps(bc.every_kind()[::3])
    for w in (1, 7):
        check(ctx, data, fixed(len(data), w), kind)


# ---- around tiles and scan blocks ----
def tile_windows(n):
    T, B = bc.tiles()
    return [w for w in (T - 1, T, T + 1, 2 * T + 31, B * T - 1, B * T + 1) if w < n]


def tile_files():
    return [(f"entry{e}", bc.entry_offset_case(e)) for e in range(32)] + bc.boundary_cases()


@pytest.mark.parametrize("name,data", tile_files(), ids=[c[0] for c in tile_files()])
def test_around_tiles_and_scan_blocks(ctx, name, data):
    assert answer(data)[0] == (bc.BAD_OP if name.endswith("count+1") else 0)
    for k, w in enumerate(tile_windows(len(data))):
        check(ctx, data, fixed(len(data), w), SOURCES[(k + len(data)) % 5])
    # two windows, cut around the first tile's end and the file's: records of every length straddle over the 32 entry cases
    T, _ = bc.tiles()
    for k, c in enumerate(c for c in (T - 17, T + 9, len(data) - 20) if 0 <= c <= len(data)):
        check(ctx, data, [c, len(data) - c], SOURCES[(k + 1 + len(data)) % 5])


def test_straddling_records_of_every_length(ctx):
    """a record of each length cut after each of its bytes, behind a tile's worth of records"""
    T, _ = bc.tiles()
    rng = np.random.default_rng(8)
    for k, length in enumerate(bc.LENGTHS):
        ops = np.concatenate([bc.fill_16_17(T - 8 - 5, rng), bc.ops_of_lengths([length, 20, 32], rng)])
        data = bc.program_file.dumps(ops)
        start = T - 5
        for c in range(start, start + length + 1):
            check(ctx, data, [c, len(data) - c], SOURCES[(c + k) % 5])


# ---- error parity ----
def first_bad_record(data):
    """(offset, length as the tags say or None) of the first record the host reader rejects, by reading record after record"""
    pos, count = 8, bc.count_of(data)
    for _ in range(count):
        if pos + 8 > len(data):
            return pos, None
        dom, opc = struct.unpack("<II", data[pos:pos + 8])
        if dom >= 4 or (dom < 2 and opc >= 10):
            return pos, None
        imm = 1 if dom == 0 else 8
        length = 20 if dom >= 2 else 8 + {0: 8, 1: 8, 2: 24, 3: 16 + imm, 4: 24, 5: 16 + imm, 6: 24, 7: 16 + imm, 8: 8, 9: 8 + imm}[opc]
        if pos + length > len(data) or bc.host_parse(bc.with_count(data[:8], 1) + data[pos:pos + length])[0]:
            return pos, length
        pos += length
    return None, None


def error_files():
    out = [(n, d) for n, d, _ in bc.single_defect_cases()] + bc.truncation_cases() + [(n, d) for n, d, _ in bc.ordering_cases()] + bc.header_cases()
    return [(n, d) for n, d in out]


@pytest.mark.parametrize("name,data", error_files(), ids=[c[0] for c in error_files()])
def test_error_parity(ctx, name, data):
    n = len(data)
    cuts = {0, min(3, n), min(8, n), n // 2, max(n - 1, 0), n}
    if n >= 8 and bc.count_of(data) <= n // 16:
        at, length = first_bad_record(data)
        if at is not None:  # before the defect, inside the defective record, behind it
            cuts |= {max(at - 3, 0), at, min(at + 5, n), min(at + (length or 8) - 1, n), min(at + (length or 8) + 4, n)}
    for k, c in enumerate(sorted(cuts)):
        check(ctx, data, [c, n - c], SOURCES[(k + n) % 5])
    if n < 4000:
        check(ctx, data, fixed(n, 33), 2)


# ---- count and tail ----
def test_count_and_tail(ctx):
    import torch

    whole = bc.program_file.dumps(bc.every_kind())
    starts, end = bc.record_starts(whole)
    n = len(starts)
    # a count below the records present, garbage behind record count - 1: not judged, fed or not
    data = bc.with_count(whole[:starts[n - 7]], n - 7) + b"\xff" * 100
    rc, _, want = bc.host_parse(data)
    assert rc == 0
    for kind in ("host", 1):
        check(ctx, data, fixed(len(data), 100), kind)
        check(ctx, data, [starts[n - 7], 100], kind)
        # ... finish is RV_OK with the host's info before the tail is fed
        src = Source(data, kind)
        with Raw(ctx, len(data)) as r:
            assert r.finish()[0] == bc.ARG
            assert r.feed(src.base, starts[n - 7] - 1, src.on_dev)[0] == 0 and r.finish()[0] == bc.ARG
            rc, piece = r.feed(src.base + starts[n - 7] - 1, 1, src.on_dev)
            assert (rc, piece["n_ops"], piece["first_op"]) == (0, 1, n - 8)
            assert r.finish() == (0, bc.expected_info(data, want))
            assert r.feed(src.base + starts[n - 7], 60, src.on_dev) == (0, {"first_op": n - 7, "n_ops": 0, "n_input_gf2": 0, "n_input_z64": 0})
            assert r.finish() == (0, bc.expected_info(data, want))
    # a count one above the records present: RV_E_BAD_OP at the feed that completes file_len
    data = bc.with_count(whole, n + 1)
    for kind in ("host", 3):
        src = Source(data, kind)
        with Raw(ctx, len(data)) as r:
            assert r.feed(src.base, len(data) - 1, src.on_dev)[0] == 0
            assert r.feed(src.base + len(data) - 1, 0, src.on_dev)[0] == 0
            assert r.feed(src.base + len(data) - 1, 1, src.on_dev)[0] == bc.BAD_OP
            assert r.finish()[0] == bc.ARG
    # a count of 0, a count no file of this length can hold: from the header, nothing of the count's size is asked of the arena
    check(ctx, bc.program_file.dumps(program([])), [3, 5], "host")
    data = bc.with_count(whole, (1 << 64) - 1)
    src = Source(data, "host")
    with Raw(ctx, len(data)) as r:
        r.feed(src.base, 100, False)  # (the arena's first blocks)
    free0 = torch.cuda.mem_get_info()[0]
    with Raw(ctx, len(data)) as r:
        assert r.feed(src.base, 7, False)[0] == 0
        assert r.feed(src.base + 7, 1, False)[0] == bc.BAD_OP
    assert free0 - torch.cuda.mem_get_info()[0] < (64 << 20)
    with Raw(ctx, 5) as r:  # no header fits
        assert r.feed(src.base, 2, False)[0] == bc.BAD_OP


# ---- arguments ----
def test_arguments(ctx):
    import torch

    data = bc.mix_of_length(3000, 41)
    rc, n, want = bc.host_parse(data)
    src = Source(data, "host")
    dev = Source(data, 1)
    with Raw(ctx, len(data)) as r:
        assert r.finish()[0] == bc.ARG  # too early
        assert r.feed(src.base, len(data) + 1, False)[0] == bc.ARG  # past file_len
        assert r.feed(0xDEAD0000, 1 << 32, True)[0] == bc.ARG  # 2^32 bytes claimed: refused before the pointer is looked at
        assert r.feed(src.base, 100, False, null_piece=True)[0] == bc.ARG
        assert r.feed(src.base, 100, True)[0] == bc.ARG  # a host pointer passed as device data
        w = 1601  # cap_ops one too small: the state is unchanged, and the same feed with enough room succeeds
        canary = torch.full((w // 16 + 2, REC), FILL, dtype=torch.uint8, device="cuda")
        assert r.feed(dev.base, w, True, canary, w // 16)[0] == bc.ARG
        torch.cuda.synchronize()
        assert bool((canary == FILL).all())
        rc, piece = r.feed(dev.base, w, True, canary, w // 16 + 1)
        upto = bisect.bisect_right(ends_of(data), w)
        assert (rc, piece["first_op"], piece["n_ops"]) == (0, 0, upto)
        assert canary[:upto].cpu().numpy().tobytes() == want[:upto * REC] and bool((canary[upto:] == FILL).all())
        assert r.feed(src.base + w, len(data) - w + 1, False)[0] == bc.ARG
        rc, piece = r.feed(src.base + w, len(data) - w, False)  # (a scan feed)
        assert (rc, piece["first_op"], piece["n_ops"]) == (0, upto, n - upto)
        assert r.finish() == (0, bc.expected_info(data, want))
        assert r.feed(src.base, 1, False)[0] == bc.ARG  # the file is over
    assert _lib.lib().rv_program_reader_finish(None, None) == bc.ARG
    _lib.lib().rv_program_reader_destroy(None)


# ---- scan feeds ----
def test_scan_feeds(ctx):
    from reverie_amd import program_file

    data = bc.mix_of_length(5000, 17)
    rc, n, want = bc.host_parse(data)
    prog = np.frombuffer(want, OP_DTYPE)
    info = program_file.scan_device(data, 100)
    wc = info.pop("wire_counts")
    assert info == bc.expected_info(data, want) and wc == (info["z64_wires"], info["gf2_wires"])
    pieces = list(program_file.iter_device(data, 100, scan=True))
    assert all(ops is None for ops, _ in pieces) and len(pieces) == 50
    for ops, piece in pieces:
        part = prog[piece["first_op"]:piece["first_op"] + piece["n_ops"]]
        for d, key in ((0, "n_input_gf2"), (1, "n_input_z64")):
            assert piece[key] == int(((part["domain"] == d) & (part["opcode"] == 0)).sum())
    assert sum(p["n_ops"] for _, p in pieces) == n
    # scan feeds and writing feeds mix within one reader
    windows = fixed(len(data), 333)
    got_rc, recs, pieces, fin = feed_all(ctx, data, windows, 2, scan={1, 2, 7})
    skipped = {i for k in (1, 2, 7) for i in range(pieces[k]["first_op"], pieces[k]["first_op"] + pieces[k]["n_ops"])}
    assert got_rc == 0 and fin == (0, bc.expected_info(data, want)) and len(skipped) > 20
    assert recs == b"".join(want[i * REC:(i + 1) * REC] for i in range(n) if i not in skipped)


# ---- offsets above 2^32 ----
def test_offsets_above_2_32(ctx):
    import torch

    body = bc.program_file.dumps(bc.every_kind())[8:]
    want = bc.every_kind().tobytes()
    n = len(want) // REC
    off, first = (1 << 32) + 7, (1 << 32) + 1
    src = Source(body, 1)
    free0 = None
    for trial in range(2):  # (the first run makes the arena's blocks)
        with Raw(ctx, (1 << 33) + 5) as r:
            assert r.resume(off, first) == 0
            recs, at = b"", 0
            for w in fixed(len(body), 300):
                d_ops = torch.full((w // 16 + 1, REC), FILL, dtype=torch.uint8, device="cuda")
                rc, piece = r.feed(src.base + at, w, True, d_ops, w // 16 + 1)
                assert rc == 0 and piece["first_op"] == first + len(recs) // REC
                recs += d_ops.cpu().numpy().tobytes()[:piece["n_ops"] * REC]
                at += w
            rc, info = r.finish()
            assert rc == 0 and recs == want
            assert info["bytes"] == off + len(body) and info["n_ops"] == first + n
        if free0 is None:
            free0 = torch.cuda.mem_get_info()[0]
    assert free0 - torch.cuda.mem_get_info()[0] < (64 << 20), "work memory grew with file_len"


# ---- end to end ----
META = json.load(open(os.path.join(GOLDEN, "proofs.json")))


def verdict(run):
    try:
        return run()
    except _lib.ReverieError as e:
        return ("err", e.code)


def evaluation(run, one):
    """("ok", ok, n_failed) of an evaluation, or (the library's code,) where it refuses"""
    try:
        r = run()
    except _lib.ReverieError as e:
        return (e.code,)
    pick = (lambda v: v[0]) if one else (lambda v: v)
    return "ok", bool(pick(r.ok)), int(pick(r.n_failed))


@pytest.mark.parametrize("name", ["adder64", "z64_mix"])
def test_end_to_end(rv, rule_seeds, name, tmp_path):
    import torch

    from reverie_amd import program_file, stream
    from reverie_amd.ops import largest_wires

    m = META[name]
    prog = program(golden_ops(m))
    w2, w64 = m["wit_gf2"], [int(x) for x in m["wit_z64"]]
    data = program_file.dumps(prog)
    wc = tuple(int(x) for x in largest_wires(prog))
    circuit = rv.Circuit(prog, wc)
    want = bytes(rv.Proof.new(circuit, w2, w64, seeds=rule_seeds))
    clear = evaluation(lambda: circuit.evaluate(w2, w64), one=False)
    assert clear[0] == ("ok" if name == "adder64" else 8)  # (z64_mix draws a Random value: no evaluator takes it)
    path = tmp_path / "program.bin"
    path.write_bytes(data)
    on_gpu = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    flipped = bytearray(want)
    flipped[len(flipped) // 2] ^= 1
    rejected = verdict(lambda: rv.Proof(bytes(flipped)).verify(circuit))  # (False, or the code of a proof that no longer parses)
    assert rejected is not True
    for source in (str(path), on_gpu):
        assert program_file.scan_device(source, 100)["wire_counts"] == wc
        got = b"".join(ops.cpu().numpy().tobytes() for ops, _ in program_file.iter_device(source, 100))
        assert got == prog.tobytes()

        def pieces():
            return program_file.iter_device(source, 100)

        for kw in ({}, {"device_compile": True, "device_z64": True, "device_b2a": True}):
            proof, info = stream.prove_streaming_pieces(pieces, w2, w64, wc, seeds=rule_seeds, **kw)
            assert bytes(proof) == want
            assert stream.verify_streaming_pieces(pieces, wc, want, **kw)[0]
            assert verdict(lambda: stream.verify_streaming_pieces(pieces, wc, bytes(flipped), **kw)[0]) == rejected
            assert evaluation(lambda: stream.evaluate_streaming_pieces(pieces, w2, w64, wc, **kw), one=True) == clear
    # host arrays that come with None: their Inputs are counted with numpy
    host_pieces = lambda: iter([(prog[:37], None), (prog[37:], None)])  # noqa: E731
    assert bytes(stream.prove_streaming_pieces(host_pieces, w2, w64, wc, seeds=rule_seeds)[0]) == want


# ---- the command line ----
def test_cli_in_child_processes(tmp_path):
    from reverie_amd import program_file

    m = META["adder64"]
    prog = program(golden_ops(m))
    (tmp_path / "adder.bin").write_bytes(program_file.dumps(prog))
    prog.tofile(tmp_path / "adder.rvops")
    (tmp_path / "wit.txt").write_text(" ".join(str(b) for b in m["wit_gf2"]))
    env = {**os.environ, "PYTHONPATH": ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")}
    bincode = ["--program-path", str(tmp_path / "adder.bin"), "--program-format", "mcircuit-bincode", "--parser", "device"]

    def run(*args):
        return subprocess.run([sys.executable, "-m", "reverie_amd"] + list(args), env=env, capture_output=True, text=True, timeout=300)

    proof = tmp_path / "proof.bin"
    r = run("--operation", "prove", "--stream", "--window-mb", "1", "--witness-path", str(tmp_path / "wit.txt"), "--proof-path", str(proof), *bincode)
    assert r.returncode == 0 and "Ok(())" in r.stdout, r.stderr[-2000:]
    for extra in (["--stream"], []):
        r = run("--operation", "verify", "--proof-path", str(proof), *extra, *bincode)
        assert r.returncode == 0 and "Ok(())" in r.stdout, r.stderr[-2000:]
    bad = bytearray(proof.read_bytes())
    bad[len(bad) // 2] ^= 1
    (tmp_path / "bad.bin").write_bytes(bytes(bad))
    r = run("--operation", "verify", "--stream", "--proof-path", str(tmp_path / "bad.bin"), *bincode)
    assert r.returncode == 1 and 'Err("Unverifiable Proof")' in r.stdout, r.stderr[-2000:]
    r = run("--operation", "oneshot-zk", "--stream", "--witness-path", str(tmp_path / "wit.txt"), "--program-path", str(tmp_path / "adder.rvops"))
    assert r.returncode == 0 and "Ok(())" in r.stdout, r.stderr[-2000:]
