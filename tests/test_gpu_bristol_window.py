"""rv_bristol_reader_* (a Bristol text read in windows on the GPU) against rv_bristol_parse on the whole text: for every way of
cutting, the records of all feeds are the host's records, every feed delivers exactly the gate lines it makes final (the Input ops
with the header, the assertion pairs with the last line), the first nonzero code is the host's and comes with the feed that owes it,
and no byte behind a window is read -- the windows are ranges of one array (host memory, or a GPU tensor at leads 0-3) that holds
the whole text, so the bytes right behind a window read as the line's continuation.  Then the Python layers (bristol.DeviceReader /
iter_device / wire_counts, stream.*_streaming_pieces) and the command line's --stream --window-mb.

The capacity every writing feed gets is the bound the header states -- the Input records still due + (held + len) / 6 + 1 +
2 * n_expected -- so every feed tests it: a MAND lane is three numbers and their blanks, six bytes of a line at the least, any other
record a whole line of eleven ("1 1 0 1 EQ" and its LF) and more; the + 1 pays for a last line without an LF."""
import bisect
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import bristol_cases as bc
import bristol_gen
from conftest import ROOT
from reverie_amd import _lib
from reverie_amd.ops import OP_DTYPE

pytestmark = pytest.mark.gpu
REC = OP_DTYPE.itemsize
FILL = 0xA5
SOURCES = ["host", 0, 1, 2, 3]  # host bytes, or a GPU tensor with the text at this lead


@pytest.fixture(scope="module")
def rv():
    import reverie_amd

    return reverie_amd


@pytest.fixture(scope="module")
def ctx(rv):
    return rv.Context.default()


def _info(bi):
    return {k: int(getattr(bi, k)) for k, _ in bi._fields_}


class Raw:
    """the C calls as they are"""

    def __init__(self, ctx, file_len, expected=None, fmt=0):
        self.h = C.c_void_p()
        e, ne = bc._exp(expected)
        assert _lib.lib().rv_bristol_reader_begin(ctx.handle, C.c_uint64(file_len), C.c_int(fmt), C.c_void_p(e.ctypes.data) if e is not None else None,
                                                  C.c_size_t(ne), C.byref(self.h)) == 0

    def feed(self, addr, n, on_dev, d_ops=None, cap=0, null_piece=False, d_addr=None):
        piece = _lib.BristolPiece()
        p_ops = d_addr if d_addr is not None else (d_ops.data_ptr() if d_ops is not None else None)
        rc = _lib.lib().rv_bristol_reader_feed(self.h, C.c_void_p(addr), C.c_size_t(n), C.c_int(1 if on_dev else 0),
                                               C.c_void_p(p_ops) if p_ops is not None else None, C.c_size_t(cap), None if null_piece else C.byref(piece))
        return rc, _info(piece)

    def header(self):
        bi = _lib.BristolInfo()
        return _lib.lib().rv_bristol_reader_header(self.h, C.byref(bi)), _info(bi)

    def finish(self):
        bi = _lib.BristolInfo()
        return _lib.lib().rv_bristol_reader_finish(self.h, C.byref(bi)), _info(bi)

    def resume(self, file_off, next_line, next_op):
        return _lib.lib().rv_hook_bristol_reader_resume(self.h, C.c_uint64(file_off), C.c_uint64(next_line), C.c_uint64(next_op))

    def close(self):
        if self.h:
            _lib.lib().rv_bristol_reader_destroy(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Source:
    """the text's bytes for the feeds: one array in host memory, or one GPU tensor (`lead` bytes, then the whole text)"""

    def __init__(self, text: bytes, kind):
        import torch

        self.on_dev = kind != "host"
        if self.on_dev:
            self.keep = torch.from_numpy(np.frombuffer(b"\xee" * kind + text + b" 7 AND\n", np.uint8).copy()).cuda()
            self.base = self.keep.data_ptr() + kind
        else:
            self.keep = np.frombuffer(text + b" 7 AND\n", np.uint8).copy()
            self.base = self.keep.ctypes.data


@functools.lru_cache(maxsize=10)
def source(text: bytes, kind):
    return Source(text, kind)


class Answer:
    """the host parser's answer for a text, computed once: code, records, info; the bytes fed at which the header is complete
    (four whole non-blank lines, or the file's end), at which gate line i < n_gates is final, and at which the code is due -- the
    first bad line is the first one the host parser rejects when it stands alone behind a header of as many wires"""

    def __init__(self, text, expected, fmt):
        import torch

        self.rc, self.n, self.recs, self.info = bc.host_parse(text, expected, fmt)
        self.want_t = None
        self.n_exp = len(expected) if expected is not None else 0
        n = len(text)
        self.header_at, lines, token = n, 0, False
        for i, c in enumerate(text):
            if c == 10:
                lines, token = lines + token, False
                if lines == 4:
                    self.header_at = i + 1
                    break
            elif c not in (32, 9, 13):
                token = True
        e, ne = bc._exp(expected)
        hi, off = _lib.BristolInfo(), C.c_size_t()
        buf = np.frombuffer(text, np.uint8) if n else np.zeros(1, np.uint8)
        self.hrc = _lib.lib().rv_internal_bristol_header(C.c_void_p(buf.ctypes.data), C.c_size_t(n), C.c_size_t(n), C.c_int(fmt), C.c_int(e is not None),
                                                         C.c_size_t(ne), C.byref(hi), C.byref(off))
        self.final_at, self.error_at, self.n_inputs, self.off = [], self.header_at, 0, 0
        if self.hrc:
            assert self.rc == self.hrc
            return
        self.n_inputs, self.off, n_gates = int(hi.n_inputs), int(off.value), int(hi.n_gates)
        p, bad = self.off, None
        while p < n and len(self.final_at) < n_gates:
            e_ = text.find(b"\n", p)
            e_ = n if e_ < 0 else e_
            line = text[p:e_]
            if line.strip(b" \t\r"):
                self.final_at.append(max(e_ + 1 if e_ < n else n, self.header_at))
                if bad is None:
                    code = bc.host_parse(b"1 %d\n1 0\n1 0\n" % hi.n_wires + line, None, 1)[0]
                    if code:
                        bad = self.final_at[-1]
                        assert code == self.rc
            p = e_ + 1
        if bad is not None:
            self.error_at = bad
        elif len(self.final_at) < n_gates:
            self.error_at = n  # the short file
        else:
            self.error_at = self.final_at[-1] if self.final_at else self.header_at  # (too many wires: with the last line)
        self.want_t = torch.from_numpy(np.frombuffer(self.recs, np.uint8).copy()).cuda().reshape(-1, REC) if not self.rc else None

    def held(self, text, at):
        """an upper bound on what the reader holds back after `at` bytes: everything before the header is complete, then the bytes
        behind the last LF (of the gate region)"""
        if at < self.header_at:
            return at
        return at - max(self.off, text.rfind(b"\n", 0, at) + 1)

    def due(self, at):
        return 0 if at < self.header_at else bisect.bisect_right(self.final_at, at)


@functools.lru_cache(maxsize=8)
def answer(text, expected, fmt):
    return Answer(text, list(expected) if expected is not None else None, fmt)


def check(ctx, text, windows, kind, expected=None, fmt=0, scan=(), fed_all=True):
    """the windows (lengths) fed in order: the host parser's answer, feed by feed.  -> the pieces"""
    import torch

    a = answer(text, tuple(expected) if expected is not None else None, fmt)
    src = source(text, kind)
    pieces, at, lines, ops, inputs_due, header_in = [], 0, 0, 0, a.n_inputs, False
    with Raw(ctx, len(text), expected, fmt) as r:
        for k, w in enumerate(windows):
            cap = inputs_due + (a.held(text, at) + w) // 6 + 1 + 2 * a.n_exp  # the bound that always suffices
            d_ops = None if k in scan else torch.full((cap + 2, REC), FILL, dtype=torch.uint8, device="cuda")
            assert r.header()[0] == (0 if header_in else bc.ARG)
            rc, piece = r.feed(src.base + at, w, src.on_dev, d_ops, cap if d_ops is not None else 0)
            at += w
            if rc:
                assert a.rc == rc, (rc, a.rc, at)
                assert a.error_at <= at and (k == 0 or at - w < a.error_at), "the code came with the wrong feed"
                # after a code the reader takes nothing more
                assert r.feed(src.base, 0, src.on_dev)[0] == bc.ARG and r.finish()[0] == bc.ARG and r.header()[0] == bc.ARG
                return pieces
            assert not a.rc or at < a.error_at, "a code is overdue"
            due = a.due(at)
            assert (piece["first_line"], piece["n_lines"], piece["first_op"]) == (lines, due - lines, ops), (piece, due, at)
            assert piece["n_input_gf2"] == (a.n_inputs if inputs_due and at >= a.header_at else 0)
            assert piece["n_ops"] <= cap
            if d_ops is not None:
                assert bool((d_ops[piece["n_ops"]:] == FILL).all()), "records behind n_ops were written"
                if not a.rc:
                    assert torch.equal(d_ops[:piece["n_ops"]], a.want_t[ops:ops + piece["n_ops"]]), (at, piece)
            if at >= a.header_at:
                inputs_due, header_in = 0, True
            lines, ops = due, ops + piece["n_ops"]
            pieces.append(piece)
        if fed_all:
            assert a.rc == 0, "the text's code never came"
        rc, info = r.finish()
        assert rc == 0 and info == a.info and ops == a.n
    return pieces


def two(n, cut):
    return [cut, n - cut]


def fixed(n, step):
    return [min(step, n - at) for at in range(0, n, step)] or [0]


def expected_for(text, fmt):
    rc, info, _ = bc.host_header(text, fmt)
    return [(3 * k + 1) & 1 for k in range(info["n_outputs"])] if rc == 0 else [1, 0]


SMALL = [(n, t, f) for n, t, f in bc.well_formed() if len(t) <= 600]


@pytest.mark.parametrize("name", [n for n, _, _ in SMALL])
def test_every_cut(ctx, name):
    """Fashion, old and ambiguous headers, CR LF, blank lines, no final LF, no gates at all (the text ends right behind the header):
    two windows at every position, with and without expected outputs, the source changing with the cut"""
    text, fmt = next((t, f) for n, t, f in SMALL if n == name)
    assert bc.host_parse(text, None, fmt)[0] == 0
    exp = expected_for(text, fmt)
    assert bc.host_parse(text, exp, fmt)[0] == 0
    for cut in range(len(text) + 1):
        check(ctx, text, two(len(text), cut), SOURCES[cut % 5], exp if cut & 1 else None, fmt)
    assert {"zero-gates", "zero-gates-no-newline", "ambiguous-old", "ambiguous-fashion", "crlf", "blanks", "no-final-newline", "old"} <= {n for n, _, _ in SMALL}


@pytest.mark.parametrize("step", [1, 7, 8, 9, 4095, 4096, 4097])
@pytest.mark.parametrize("kind", SOURCES)
def test_small_windows(ctx, kind, step):
    """random netlists of one tile and a byte and of two tiles, fed `step` bytes at a time (one byte at a time: the first alone, from
    host memory and from a tensor, for the time 8192 feeds take)"""
    tile, _ = bc.tiles()
    assert tile == 4096
    if step == 1 and kind not in ("host", 3):
        step = 2
    for text in (bc.of_length(tile + 1, 31), bc.of_length(2 * tile, 32))[:1 if step <= 2 else 2]:
        assert bc.host_parse(text)[0] == 0
        check(ctx, text, fixed(len(text), step), kind, expected_for(text, 0) if step & 1 else None)


@pytest.mark.parametrize("kind", SOURCES)
def test_a_workgroup_of_lines_in_one_feed(ctx, kind):
    """256 and 257 lines made final by one feed, behind a first feed that ends inside a line"""
    _, wg = bc.tiles()
    for n in (wg, wg + 1):
        text = bc.random_netlist(n + 1, 40 + n)
        a = answer(text, None, 0)
        assert a.rc == 0 and len(a.final_at) == n + 1
        cut = a.final_at[0] + 3
        assert check(ctx, text, two(len(text), cut), kind)[1]["n_lines"] == n
        check(ctx, text, [cut, a.final_at[-1] - 1 - cut, 1], kind, expected_for(text, 0))


@pytest.mark.parametrize("kind", ["host", 1])
def test_long_lines(ctx, kind):
    tile, _ = bc.tiles()
    text = bc.long_mand(tile // 2)  # one line of more than two tiles
    assert bc.host_parse(text)[0] == 0 and len(text) > 2 * tile
    for step in (1000, tile, tile + 1):
        pieces = check(ctx, text, fixed(len(text), step), kind, expected_for(text, 0))
        assert sum(p["n_lines"] == 0 for p in pieces) >= 2  # the line spans several windows
    lines, w = bc.random_lines(6, 3)
    blanks = bc.fashion(8, 2, w, lines, sep=b"\n" + b" \t\r " * (tile // 2) + b"\n")  # runs of whitespace longer than two tiles
    assert bc.host_parse(blanks)[0] == 0
    for step in (999, tile):
        check(ctx, blanks, fixed(len(blanks), step), kind)


ERRORS = bc.error_texts()


@pytest.mark.parametrize("name", [e[0] for e in ERRORS])
def test_error_parity(ctx, name):
    _, text, exp, fmt, code = next(e for e in ERRORS if e[0] == name)
    assert bc.host_parse(text, exp, fmt)[0] == code
    a = answer(text, tuple(exp) if exp is not None else None, fmt)
    n = len(text)
    cuts = sorted({0, 1, n // 2, n - 1, n, a.header_at, a.error_at - 1, a.error_at, min(n, a.error_at + 1), a.header_at - 1} & set(range(n + 1)))
    for k, cut in enumerate(cuts):
        check(ctx, text, two(n, cut), SOURCES[k % 5], exp, fmt)
    if n <= 4 * bc.tiles()[0]:
        check(ctx, text, fixed(n, 5), "host", exp, fmt)
        check(ctx, text, fixed(n, 64), 2, exp, fmt, scan={0, 2, 3})


def test_garbage_behind_the_last_line(ctx):
    text = next(t for n, t, _ in bc.well_formed() if n == "trailing-garbage")
    a = answer(text, None, 0)
    assert a.rc == 0 and a.final_at[-1] < len(text) - 10
    for kind in ("host", 2):
        for cut in (a.final_at[-1] - 1, a.final_at[-1], a.final_at[-1] + 5):
            check(ctx, text, two(len(text), cut), kind)
        # not fed at all: finish is RV_OK once the last gate line is final
        src = source(text, kind)
        with Raw(ctx, len(text)) as r:
            assert r.finish()[0] == bc.ARG
            rc, piece = r.feed(src.base, a.final_at[-1] - 1, src.on_dev)
            assert rc == 0 and r.finish()[0] == bc.ARG
            rc, piece = r.feed(src.base + a.final_at[-1] - 1, 1, src.on_dev)
            assert rc == 0 and piece["n_lines"] == 1 and r.finish() == (0, a.info)


def test_capacity_rule(ctx):
    import torch

    text = bc.random_netlist(60, 9, mand_every=4)
    exp = expected_for(text, 0)
    a = answer(text, tuple(exp), 0)
    assert a.rc == 0
    for kind in ("host", 3):
        src = source(text, kind)
        with Raw(ctx, len(text), exp) as r:
            at, ops = 0, 0
            for w in fixed(len(text), 400):
                d_ops = torch.full((400, REC), FILL, dtype=torch.uint8, device="cuda")
                rc, piece = r.feed(src.base + at, w, src.on_dev, d_ops, 1)
                n = piece["n_ops"]
                assert rc == bc.ARG and n > 1, "one record's room cannot do for 400 bytes of gate lines"
                assert bool((d_ops == FILL).all()), "a feed that does not fit wrote"
                assert r.feed(src.base + at, w, src.on_dev, d_ops, n - 1)[0] == bc.ARG and bool((d_ops == FILL).all())
                rc, piece = r.feed(src.base + at, w, src.on_dev, d_ops, n)  # the same bytes again, with the count named
                assert rc == 0 and piece["n_ops"] == n and piece["first_op"] == ops
                assert torch.equal(d_ops[:n], a.want_t[ops:ops + n]) and bool((d_ops[n:] == FILL).all())
                at, ops = at + w, ops + n
            assert r.finish() == (0, a.info) and ops == a.n


def test_scan_feeds(ctx):
    text = bc.random_netlist(300, 21, mand_every=7)
    exp = expected_for(text, 0)
    for kind in ("host", 1):
        pieces = check(ctx, text, fixed(len(text), 333), kind, exp, scan={0, 1, 4, 9})
        assert sum(p["n_ops"] for p in pieces) == answer(text, tuple(exp), 0).n


def test_argument_list(ctx):
    import torch

    text = bc.random_netlist(20, 4)
    src, dev = source(text, "host"), source(text, 0)
    d_ops = torch.full((100, REC), FILL, dtype=torch.uint8, device="cuda")
    host_ops = np.zeros((100, REC), np.uint8)
    with Raw(ctx, len(text)) as r:
        assert r.feed(src.base, 10, False, null_piece=True)[0] == bc.ARG
        assert r.feed(None, 10, False)[0] == bc.ARG
        assert _lib.lib().rv_bristol_reader_feed(None, C.c_void_p(src.base), C.c_size_t(1), C.c_int(0), None, C.c_size_t(0), C.byref(_lib.BristolPiece())) == bc.ARG
        assert r.feed(src.base, 1 << 32, False)[0] == bc.ARG
        assert r.feed(src.base, len(text) + 1, False)[0] == bc.ARG  # past file_len
        assert r.feed(src.base, 10, False, d_addr=d_ops.data_ptr() + 4, cap=10)[0] == bc.ARG  # misaligned
        assert r.feed(src.base, 10, False, d_addr=host_ops.ctypes.data, cap=10)[0] == bc.ARG  # no device memory
        assert r.feed(src.base, 10, False, d_ops, 1 << 30)[0] == bc.ARG  # more rows than the allocation has (a pooled block: far more)
        assert r.feed(src.base, 10, True)[0] == bc.ARG  # host memory given as a device text
        with Raw(ctx, 1 << 33) as big:  # (a file long enough for the feed: the allocation is what is too short)
            assert big.feed(dev.base, 1 << 31, True)[0] == bc.ARG and big.feed(dev.base, len(text), True)[0] == 0
        assert bool((d_ops == FILL).all())
        assert r.header()[0] == bc.ARG and r.finish()[0] == bc.ARG
        # none of them moved the reader
        rc, piece = r.feed(src.base, len(text), False, d_ops, 100)
        a = answer(text, None, 0)
        assert rc == 0 and piece["n_ops"] == a.n and torch.equal(d_ops[:a.n], a.want_t) and r.finish() == (0, a.info)
        assert r.feed(src.base, 1, False)[0] == bc.ARG  # the file is fed
    assert _lib.lib().rv_bristol_reader_begin(ctx.handle, 8, 0, None, 0, None) == bc.ARG


def test_counters_above_2_32(ctx):
    import torch

    lines, w = bc.random_lines(50, 77, mand_every=6)
    small = bc.fashion(8, 2, w, lines)
    exp = expected_for(small, 0)
    rc, n, want, info = bc.host_parse(small, exp, 0)
    assert rc == 0
    _, _, off = bc.host_header(small)
    tail = small[off:]
    before, first = (1 << 31) + 11, (1 << 33) + 5  # (a header number stays below 2^32; the file offset and the ordinals do not)
    head = b"%d %d\n1 8\n1 2\n" % (before + len(lines), w)
    file_len = 8 * (before + len(lines)) + 4096
    src, hsrc = Source(tail, 1), Source(head, "host")
    free0 = None
    for trial in range(2):  # (the first run makes the arena's blocks)
        with Raw(ctx, file_len, exp, 1) as r:
            assert r.feed(hsrc.base, len(head), False)[0] == 0 and r.header()[0] == bc.ARG  # the header lines alone: not yet judged
            assert r.resume(file_len - len(tail), before, first) == 0
            rc, hdr = r.header()
            assert rc == 0 and hdr["n_gates"] == before + len(lines) and hdr["gf2_wires"] == w + 2
            recs, at, ln = b"", 0, before
            for wlen in fixed(len(tail), 300):
                d_ops = torch.full((wlen // 6 + 60, REC), FILL, dtype=torch.uint8, device="cuda")
                rc, piece = r.feed(src.base + at, wlen, True, d_ops, wlen // 6 + 60)
                assert rc == 0 and piece["first_op"] == first + len(recs) // REC and piece["first_line"] == ln and piece["n_input_gf2"] == 0
                recs += d_ops.cpu().numpy().tobytes()[:piece["n_ops"] * REC]
                at, ln = at + wlen, ln + piece["n_lines"]
            assert r.finish()[0] == 0 and ln == before + len(lines)
            assert recs == want[8 * REC:]  # (the eight Input records went with the header)
        if free0 is None:
            free0 = torch.cuda.mem_get_info()[0]
    assert free0 - torch.cuda.mem_get_info()[0] < (64 << 20), "work memory grew with file_len or n_gates"


def test_iter_device_and_wire_counts(ctx, tmp_path):
    import torch

    from reverie_amd import bristol

    text = bc.random_netlist(400, 5, n_in=64, mand_every=9)
    exp = expected_for(text, 0)
    prog, info = bristol.parse(text, exp)
    path = tmp_path / "netlist.txt"
    path.write_bytes(text)
    on_gpu = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda()
    for src in (str(path), text, on_gpu):
        assert bristol.wire_counts(src, exp) == info["wire_counts"] and bristol.wire_counts(src) == (0, info["n_wires"])
        done = {}
        pieces = list(bristol.iter_device(src, 1000, exp, info=done))
        assert len(pieces) == -(-len(text) // 1000) and done == info
        assert b"".join(ops.cpu().numpy().tobytes() for ops, _ in pieces) == prog.tobytes()
        assert [p["n_input_gf2"] for _, p in pieces] == [info["n_inputs"]] + [0] * (len(pieces) - 1) and all(p["n_input_z64"] == 0 for _, p in pieces)
        done = {}
        assert all(ops is None for ops, _ in bristol.iter_device(src, 777, exp, scan=True, info=done)) and done == info
    with pytest.raises(_lib.ReverieError) as e:
        bristol.wire_counts(text, exp + [1])
    assert e.value.code == bc.ARG
    with bristol.DeviceReader(len(text), exp) as r:  # the reader repeats a feed that needs more room than len // 6 + 1
        ops, piece = r.feed(text[:60])
        assert piece["n_ops"] >= info["n_inputs"] == 64 > 60 // 6 + 1
        assert r.header()["n_gates"] == info["n_gates"]
        ops2, _ = r.feed(text[60:])
        assert ops.cpu().numpy().tobytes() + ops2.cpu().numpy().tobytes() == prog.tobytes() and r.finish() == info


@pytest.mark.parametrize("name", ["adder64", "aes128"])
def test_end_to_end(rv, rule_seeds, name):
    from reverie_amd import bristol, stream

    text = getattr(bristol_gen, name)().encode()
    plain, pinfo = bristol.parse(text)
    rng = np.random.default_rng(5)
    wit = [int(x) for x in rng.integers(0, 2, pinfo["n_inputs"])]
    values = bristol_gen.evaluate(plain, wit)
    exp = values[pinfo["n_wires"] - pinfo["n_outputs"]:pinfo["n_wires"]]
    prog, info = bristol.parse(text, exp)
    wc = info["wire_counts"]
    assert bristol.wire_counts(text, exp) == wc
    circuit = rv.Circuit(prog, wc)
    want = bytes(rv.Proof.new(circuit, wit, [], seeds=rule_seeds))

    def pieces():
        return bristol.iter_device(text, 4096, exp)

    assert b"".join(ops.cpu().numpy().tobytes() for ops, _ in pieces()) == prog.tobytes()
    proof, _ = stream.prove_streaming_pieces(pieces, wit, [], wc, seeds=rule_seeds)
    assert bytes(proof) == want
    assert stream.verify_streaming_pieces(pieces, wc, want)[0]
    r = stream.evaluate_streaming_pieces(pieces, wit, [], wc)
    clear = circuit.evaluate(wit, [])
    assert bool(r.ok[0]) and bool(clear.ok) and int(r.n_failed[0]) == 0
    wrong = list(exp)
    wrong[0] ^= 1
    r = stream.evaluate_streaming_pieces(lambda: bristol.iter_device(text, 4096, wrong), wit, [], wc)
    assert not bool(r.ok[0]) and int(r.n_failed[0]) == 1


def test_cli_in_child_processes(tmp_path):
    a, b = 0x0123456789ABCDEF, 0xFEDCBA9876543210
    (tmp_path / "adder.txt").write_text(bristol_gen.adder64())
    (tmp_path / "wit.txt").write_text(" ".join(str((a >> i) & 1) for i in range(64)) + "\n" + " ".join(str((b >> i) & 1) for i in range(64)))
    (tmp_path / "exp.txt").write_text("".join(str((((a + b) & (2**64 - 1)) >> i) & 1) for i in range(64)))
    env = {**os.environ, "PYTHONPATH": ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")}
    program = ["--program-path", str(tmp_path / "adder.txt"), "--expected-outputs-path", str(tmp_path / "exp.txt"), "--parser", "device"]

    def run(*args):
        return subprocess.run([sys.executable, "-m", "reverie_amd"] + list(args), env=env, capture_output=True, text=True, timeout=300)

    proof = tmp_path / "proof.bin"
    r = run("--operation", "prove", "--stream", "--window-mb", "1", "--witness-path", str(tmp_path / "wit.txt"), "--proof-path", str(proof), *program)
    assert r.returncode == 0 and "Ok(())" in r.stdout, r.stderr[-2000:]
    for extra in (["--stream", "--window-mb", "1"], ["--stream"], []):
        r = run("--operation", "verify", "--proof-path", str(proof), *extra, *program)
        assert r.returncode == 0 and "Ok(())" in r.stdout, r.stderr[-2000:]
    r = run("--operation", "oneshot", "--evaluator", "stream", "--window-mb", "1", "--witness-path", str(tmp_path / "wit.txt"), *program)
    assert r.returncode == 0 and "()" in r.stdout, r.stderr[-2000:]
