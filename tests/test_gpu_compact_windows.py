"""rv_compactor_* (csrc/compact_win.hip: wire compaction of a list read in windows) against the host sweep rv_ops_compact_wires,
records and info byte for byte, for every way of cutting the two passes that the carried state can go wrong at; the order of calls,
the checks that a pass is the scanned list, the error codes feed by feed, the memory figures; then what it is for: a Bristol text
and a program file read in windows, compacted in windows and proved, verified and evaluated as streams."""
import ctypes as C

import numpy as np
import pytest

import circuits
import compact_cases
from reverie_amd.ops import B2A, DOM_B2A, GF2, OP_DTYPE, Z64, SizeHint, program

pytestmark = pytest.mark.gpu

OP_BYTES = OP_DTYPE.itemsize
T = compact_cases.TILE
PAD = 88  # bytes behind a feed's records in its output tensor (no multiple of the record size)
E_ARG = 9
CORPUS = compact_cases.corpus()
BY_NAME = {c[0]: c for c in CORPUS}
ERRORS = compact_cases.error_cases()
INFO_FIELDS = ("z64_wires", "gf2_wires", "gf2_pinned", "gf2_zero_wire", "z64_zero_wire", "gf2_values", "z64_values")
MODES = ("host", "device", "in_place")
_SWEEPS = {}


@pytest.fixture(scope="module")
def rv():
    import reverie_amd

    reverie_amd.Context.default()
    return reverie_amd


def sweep(prog, wc, key=None):
    """-> (rc, records, info) of the host sweep (kept per named case)"""
    from reverie_amd import _lib

    if key is not None and key in _SWEEPS:
        return _SWEEPS[key]
    prog = np.ascontiguousarray(prog)
    out, ci = np.empty_like(prog), _lib.CompactInfo()
    rc = _lib.lib().rv_ops_compact_wires(prog.ctypes.data_as(C.c_void_p), len(prog), int(wc[0]), int(wc[1]), out.ctypes.data_as(C.c_void_p), C.byref(ci))
    r = (rc, out.tobytes() if rc == 0 else None, {k: int(getattr(ci, k)) for k in INFO_FIELDS} if rc == 0 else None)
    if key is not None:
        _SWEEPS[key] = r
    return r


class Win:
    """rv_compactor through ctypes, every call answering its code"""

    def __init__(self, rv, wc):
        from reverie_amd import _lib

        self.L, self.lib = _lib.lib(), _lib
        self.h = C.c_void_p()
        assert self.L.rv_compactor_begin(rv.Context.default().handle, int(wc[0]), int(wc[1]), C.byref(self.h)) == 0

    @staticmethod
    def _device(part, pad=0):
        import torch

        t = torch.full((len(part) * OP_BYTES + pad,), 0xA5, dtype=torch.uint8, device="cuda")
        if len(part):
            t[:len(part) * OP_BYTES] = torch.from_numpy(np.ascontiguousarray(part).view(np.uint8).reshape(-1).copy()).cuda()
        torch.cuda.synchronize()
        return t

    def scan(self, part, mode="host"):
        part = np.ascontiguousarray(part)
        if mode == "host":
            return self.L.rv_compactor_scan(self.h, part.ctypes.data_as(C.c_void_p) if len(part) else None, len(part), 0)
        t = self._device(part)
        rc = self.L.rv_compactor_scan(self.h, C.c_void_p(t.data_ptr()), len(part), 1)
        assert t.cpu().numpy().tobytes() == part.tobytes()  # (a scan reads only)
        return rc

    def scan_end(self):
        again, ci = C.c_int(-1), self.lib.CompactInfo()
        rc = self.L.rv_compactor_scan_end(self.h, C.byref(again), C.byref(ci))
        return rc, again.value, {k: int(getattr(ci, k)) for k in INFO_FIELDS}

    def feed(self, part, mode="host"):
        """-> (rc, the feed's records); the bytes behind them must be untouched"""
        part = np.ascontiguousarray(part)
        n = len(part)
        if mode == "in_place":
            t = self._device(part, PAD)
            rc = self.L.rv_compactor_feed(self.h, C.c_void_p(t.data_ptr()), n, 1, C.c_void_p(t.data_ptr()))
            got = t.cpu().numpy()
        else:
            out = self._device(part[:0], n * OP_BYTES + PAD)
            if mode == "host":
                rc = self.L.rv_compactor_feed(self.h, part.ctypes.data_as(C.c_void_p) if n else None, n, 0, C.c_void_p(out.data_ptr()))
            else:
                t = self._device(part)
                rc = self.L.rv_compactor_feed(self.h, C.c_void_p(t.data_ptr()), n, 1, C.c_void_p(out.data_ptr()))
                assert t.cpu().numpy().tobytes() == part.tobytes()
            got = out.cpu().numpy()
        assert got[n * OP_BYTES:].tobytes() == b"\xA5" * PAD
        return rc, got[:n * OP_BYTES].tobytes()

    def rewind(self):
        return self.L.rv_compactor_rewind(self.h)

    def info(self):
        ci = self.lib.CompactorInfo()
        rc = self.L.rv_compactor_get_info(self.h, C.byref(ci))
        return rc, {k: int(getattr(ci, k)) for k, _ in ci._fields_}

    def close(self):
        self.L.rv_compactor_destroy(self.h)
        self.h = C.c_void_p()


def parts(prog, cuts):
    edges = [0] + sorted(int(c) for c in cuts) + [len(prog)]
    return [prog[a:b] for a, b in zip(edges[:-1], edges[1:])]


def run(rv, prog, wc, scan_cuts=(), feed_cuts=(), passes=1, modes=MODES):
    """-> (records per rewrite pass, rv_compact_info, rv_compactor_info, scan passes made); every code must be RV_OK"""
    w = Win(rv, wc)
    try:
        scans = 0
        while True:
            for k, part in enumerate(parts(prog, scan_cuts)):
                assert w.scan(part, modes[k % len(modes)] if modes[k % len(modes)] != "in_place" else "device") == 0
            rc, again, info = w.scan_end()
            assert rc == 0 and again in (0, 1)
            scans += 1
            if not again:
                break
        outs = []
        for p in range(passes):
            if p:
                assert w.rewind() == 0
            got = []
            for k, part in enumerate(parts(prog, feed_cuts)):
                rc, rec = w.feed(part, modes[(k + 1) % len(modes)])
                assert rc == 0
                got.append(rec)
            outs.append(b"".join(got))
        rc, cinfo = w.info()
        assert rc == 0 and cinfo["total_ops"] == len(prog) and cinfo["scans"] == scans
        return outs, info, cinfo, scans
    finally:
        w.close()


def check(rv, name, prog, wc, scan_cuts=(), feed_cuts=(), passes=1, modes=MODES):
    rc, want, info = sweep(prog, wc, name)
    assert rc == 0
    outs, got_info, cinfo, scans = run(rv, prog, wc, scan_cuts, feed_cuts, passes, modes)
    for out in outs:
        assert out == want
    assert got_info == info
    has_b2a = bool((prog["domain"] == DOM_B2A).any())
    assert scans == (2 if has_b2a else 1) and cinfo["b2a"] == int(has_b2a)
    return cinfo


def random_cuts(rng, n, k):
    """k offsets in [0, n], some of them twice (empty feeds lie between)"""
    c = sorted(rng.integers(0, n + 1, k).tolist()) if n else [0] * k
    return sorted(c + c[:2])


@pytest.mark.parametrize("name,prog,wc", CORPUS, ids=[c[0] for c in CORPUS])
def test_corpus_whole_and_in_random_cuts(rv, name, prog, wc):
    check(rv, name, prog, wc)
    rng = np.random.default_rng(len(prog) + 1)
    check(rv, name, prog, wc, random_cuts(rng, len(prog), 5), random_cuts(rng, len(prog), 7))


@pytest.mark.parametrize("name", ["a_equals_b", "assert_last_reader", "zero_reads", "sizehints", "b2a_ranges", "chain40", "all_dead"])
def test_op_by_op(rv, name):
    _, prog, wc = BY_NAME[name]
    every = range(1, len(prog))
    check(rv, name, prog, wc, every, every, modes=("host",))
    check(rv, name, prog, wc, (), every, modes=("device",))
    check(rv, name, prog, wc, every, (), modes=("host",))


def test_every_release_crosses_the_cut(rv):
    _, prog, wc = BY_NAME["all_fresh"]
    check(rv, "all_fresh", prog, wc, [300], [300])
    check(rv, "all_fresh", prog, wc, [299], [301])


@pytest.mark.parametrize("n", [T - 1, T, T + 1, 2 * T + 1])
def test_cuts_around_a_workgroup(rv, n):
    prog, wc = compact_cases.of_length(n, seed=n)
    around = [c for k in range(1, 3) for c in (T * k - 1, T * k, T * k + 1) if c <= n]
    check(rv, "of_length_%d" % n, prog, wc, [T * k for k in range(1, 3) if T * k <= n], around)
    check(rv, "of_length_%d" % n, prog, wc, around, [n // 2])


def test_bench70k_cut_around_every_workgroup(rv):
    _, prog, wc = BY_NAME["golden_bench70k"]
    n = len(prog)
    around = [c for k in range(1, n // T + 1) for c in (T * k - 1, T * k, T * k + 1) if c <= n]
    check(rv, "golden_bench70k", prog, wc, [T * k for k in range(1, n // T + 1)], around, modes=("device", "in_place"))


def test_reuse_chain_across_feeds(rv):
    """chain(5000) in feeds of 1024: every slot but two comes from the carried queue, the chain never breaks at a cut"""
    prog, wc = compact_cases.chain(5000)
    cuts = range(1024, len(prog), 1024)
    check(rv, "chain5000", prog, wc, cuts, cuts)
    check(rv, "chain5000", prog, wc, (), range(1000, len(prog), 1000))


def shapes():
    k = 64
    filler = [GF2.Add(10 + (i % 7), 1, 2) for i in range(k)]
    out = []
    # a value defined in the first feed and last read in the last one
    ops = [GF2.Input(0), GF2.Input(1), GF2.Input(2)] + filler + filler + [GF2.Mul(3, 0, 1), GF2.AssertZero(3)]
    out.append(("first_to_last", program(ops), (0, 20), [3, 3 + k, 3 + 2 * k]))
    # an index redefined in every feed (and read across each cut)
    ops = [GF2.Input(0), GF2.Input(5)]
    for f in range(6):
        ops += [GF2.Add(6, 5, 0), GF2.Mul(5, 6, 6), GF2.Add(0, 5, 6), GF2.AddConst(5, 5, 1)]
    out.append(("redefined_every_feed", program(ops + [GF2.AssertZero(5)]), (0, 7), [2 + 4 * f for f in range(1, 6)]))
    # the first zero-wire read in the last feed only: the pool base of the first feed already includes the reserved wire
    ops = [GF2.Input(0), Z64.Input(0)] + filler[:20] + [Z64.Add(1, 0, 0), Z64.Mul(2, 1, 0)] + [GF2.Add(4, 0, 9), Z64.Add(3, 2, 7), GF2.AssertZero(4)]
    out.append(("late_zero_read", program(ops), (8, 20), [2, 12, 24]))
    # a SizeHint that raises both counts in a middle feed (the tables grow with their contents kept)
    ops = [GF2.Input(0), GF2.Input(1), Z64.Input(0), GF2.Mul(2, 0, 1), SizeHint(40, 300), GF2.Add(290, 2, 0), Z64.Add(39, 0, 0), GF2.Mul(3, 290, 2),
           Z64.Mul(1, 39, 0), SizeHint(41, 10), GF2.AssertZero(3), Z64.AssertZero(1)]
    out.append(("hint_in_the_middle", program(ops), (1, 3), [3, 6, 9]))
    # a B2A op only in the last feed: the indices it pins were pool indices in every earlier feed of the first scan
    ops = [GF2.Input(i) for i in range(70)] + [GF2.Add(70 + i, i, i + 1) for i in range(20)] + [GF2.Mul(3, 70, 71), B2A(0, 2), Z64.AssertZero(0)]
    out.append(("b2a_in_the_last_feed", program(ops), (1, 100), [30, 70, 91]))
    return out


SHAPES = shapes()


@pytest.mark.parametrize("name,prog,wc,cuts", SHAPES, ids=[s[0] for s in SHAPES])
def test_carried_state_shapes(rv, name, prog, wc, cuts):
    check(rv, name, prog, wc)
    check(rv, name, prog, wc, cuts, cuts)
    check(rv, name, prog, wc, cuts, [c + 1 for c in cuts])
    check(rv, name, prog, wc, range(1, len(prog)), range(1, len(prog)), modes=("host",))


def test_rewind_repeats_the_pass(rv):
    for name in ("golden_adder64", "random_mixed_3", "b2a_ranges"):
        _, prog, wc = BY_NAME[name]
        check(rv, name, prog, wc, [len(prog) // 3], [len(prog) // 2, len(prog) // 2 + 1], passes=3)


def test_order_of_calls(rv):
    _, prog, wc = BY_NAME["b2a_ranges"]
    _, want, info = sweep(prog, wc, "b2a_ranges")
    w = Win(rv, wc)
    try:
        assert w.feed(prog)[0] == E_ARG and w.rewind() == E_ARG
        assert w.scan(prog[:20]) == 0 and w.scan(prog[20:], "device") == 0
        assert w.scan_end()[:2] == (0, 1)
        # the rescan may not be skipped, cut short or run long
        assert w.feed(prog)[0] == E_ARG and w.rewind() == E_ARG
        assert w.scan_end()[0] == E_ARG
        assert w.scan(prog[:40]) == 0 and w.scan_end()[0] == E_ARG
        assert w.scan(prog[40:].repeat(2)) == E_ARG  # (beyond the first scan's count: nothing moved)
        assert w.scan(prog[40:]) == 0
        rc, again, got = w.scan_end()
        assert (rc, again) == (0, 0) and got == info
        assert w.info()[1]["scans"] == 2
        assert w.scan(prog) == E_ARG and w.scan_end()[0] == E_ARG and w.rewind() == E_ARG  # (no pass to rewind yet)
        rc, first = w.feed(prog[:10])
        assert rc == 0 and w.rewind() == E_ARG  # (a short pass is not rewound)
        assert w.feed(prog)[0] == E_ARG  # (beyond the count)
        rc, rest = w.feed(prog[10:], "device")
        assert rc == 0 and first + rest == want
        assert w.feed(prog[:1])[0] == E_ARG and w.feed(prog[:0])[0] == 0
        assert w.rewind() == 0 and w.feed(prog, "in_place") == (0, want)
    finally:
        w.close()


@pytest.mark.parametrize("what", ["altered", "short", "long"])
def test_a_pass_must_be_the_scanned_list(rv, what):
    _, prog, wc = BY_NAME["random_mixed_1"]  # (B2A ops: a rescan, then the rewrite pass)
    other = prog.copy()
    other["imm"][len(prog) // 2] ^= 1  # (the digest covers every field; the liveness does not depend on this one)
    for in_rescan in (True, False):
        w = Win(rv, wc)
        try:
            assert w.scan(prog) == 0 and w.scan_end()[:2] == (0, 1)
            if in_rescan:
                if what == "altered":
                    assert w.scan(other[:100]) == 0 and w.scan(other[100:]) == 0 and w.scan_end()[0] == E_ARG
                elif what == "short":
                    assert w.scan(prog[:-1]) == 0 and w.scan_end()[0] == E_ARG
                else:
                    assert w.scan(prog) == 0 and w.scan(prog[:1]) == E_ARG
                continue
            assert w.scan(prog[:300]) == 0 and w.scan(prog[300:]) == 0 and w.scan_end()[:2] == (0, 0)
            if what == "altered":
                assert w.feed(other[:100])[0] == 0 and w.feed(other[100:])[0] == E_ARG
            elif what == "short":
                assert w.feed(prog[:-1])[0] == 0 and w.rewind() == E_ARG
            else:
                assert w.feed(prog)[0] == 0 and w.feed(prog[:1])[0] == E_ARG
        finally:
            w.close()


@pytest.mark.parametrize("name,prog,wc,code", ERRORS, ids=[e[0] for e in ERRORS])
def test_error_codes_feed_by_feed(rv, name, prog, wc, code):
    want = sweep(prog, wc)[0]
    assert want != 0 and (code is None or code == want)
    from compact_ref import validate

    bad = next(i for i in range(len(prog)) if validate(prog[:i + 1], *wc))  # the first bad op
    for lo, hi in ((bad, len(prog)), (0, bad + 1), (bad, bad + 1), (0, len(prog))):  # the bad op first, last, alone; the list whole
        for mode in ("host", "device"):
            w = Win(rv, wc)
            try:
                assert w.scan(prog[:lo], mode) == 0  # (not earlier)
                assert w.scan(prog[lo:hi], mode) == want
                assert w.scan(prog[hi:], mode) == E_ARG and w.scan(prog[:0]) == E_ARG and w.scan_end()[0] == E_ARG
                assert w.feed(prog[:1])[0] == E_ARG and w.rewind() == E_ARG and w.info()[0] == E_ARG
            finally:
                w.close()


def test_memory_follows_the_feed_and_the_old_wire_counts(rv):
    for name in ("layered_gf2_ssa", "golden_bench70k"):
        _, prog, wc = BY_NAME[name]
        _, _, info = sweep(prog, wc, name)
        whole = check(rv, name, prog, wc, modes=("device",))
        cuts = range(2048, len(prog), 2048)
        small = check(rv, name, prog, wc, cuts, cuts, modes=("device",))
        bound = 8 * (wc[0] + wc[1]) + 8 * wc[1] * small["b2a"] + len(prog) + 4 * (info["z64_wires"] + info["gf2_wires"]) + 4096
        print(name, "state_bytes", small["state_bytes"], "bound", bound, "peak_feed_bytes", small["peak_feed_bytes"], "whole", whole["peak_feed_bytes"])
        assert small["state_bytes"] <= bound and whole["state_bytes"] <= bound
        if name == "golden_bench70k":
            assert small["peak_feed_bytes"] <= whole["peak_feed_bytes"] // 8


# ---- what it is for ----
def ev(r):
    return tuple(np.atleast_1d(np.asarray(v)).tolist() for v in (r.ok, r.n_failed, r.first_failed_op))


def evaluation(rv, run):
    try:
        return ev(run())
    except rv.ReverieError as e:
        return "refused", e.code


def same_pieces_of_the_whole_list(stream, prog, wc, pieces, w2, w64, seeds):
    """-> (proof, info) of the list compacted whole (compact_wires) and streamed in the pieces the windows cut.  rv_stream_info's
    wire_store_bytes counts the wire rows and the largest chunk's rows, so it is compared between streams that are cut alike."""
    from reverie_amd import compact

    small, new_wc, cinfo = compact.compact_wires(prog, wc)
    edges = np.cumsum([0] + [0 if ops is None else len(ops) for ops, _ in pieces()])
    assert edges[-1] == len(prog)
    proof, info = stream.prove_streaming_pieces(lambda: iter([(small[a:b], None) for a, b in zip(edges[:-1], edges[1:])]), w2, w64, new_wc, seeds=seeds)
    return proof, dict(info, compact=cinfo)


def test_bristol_text_in_windows_to_a_streamed_proof(rv, rule_seeds):
    from reverie_amd import bristol, stream

    full, wit, _, _ = circuits.layered_gf2(64, 256, 12, fold_to=16)
    exp = [int(x) for x in full["imm"][-32::2]]  # (the tail's AddConst constants: the clear outputs)
    text = bristol.dumps(full[:-32], n_outputs=16)
    prog, info = bristol.parse(text, exp)
    wc = info["wire_counts"]
    want = bytes(rv.Proof.new(prog, wit, [], wc, seeds=rule_seeds))

    def pieces():
        return bristol.iter_device(text, 4096, exp)

    assert sum(1 for _ in pieces()) > 10
    proof, got = stream.prove_streaming_pieces(pieces, wit, [], wc, seeds=rule_seeds, compact_wires=True)
    assert bytes(proof) == want
    _, whole = same_pieces_of_the_whole_list(stream, prog, wc, pieces, wit, [], rule_seeds)
    _, plain = stream.prove_streaming_pieces(pieces, wit, [], wc, seeds=rule_seeds)
    assert got["compact"] == dict(whole["compact"], compactor=got["compact"]["compactor"]) and got["compact"]["compactor"]["scans"] == 1
    assert got["wire_store_bytes"] == whole["wire_store_bytes"] < plain["wire_store_bytes"] and "compact" not in plain
    assert got["wire_store_bytes"] <= stream.prove_streaming(prog, wit, [], wc, seeds=rule_seeds, compact_wires=True)[1]["wire_store_bytes"]
    ok, vinfo = stream.verify_streaming_pieces(pieces, wc, want, compact_wires=True)
    assert ok and vinfo["wire_store_bytes"] < plain["wire_store_bytes"]
    flipped = bytearray(want)
    flipped[len(flipped) // 2] ^= 1
    try:
        assert not stream.verify_streaming_pieces(pieces, wc, bytes(flipped), compact_wires=True)[0]
    except rv.ReverieError:
        pass
    einfo = {}
    r = stream.evaluate_streaming_pieces(pieces, wit, [], wc, compact_wires=True, info=einfo)
    clear = stream.evaluate_streaming(prog, wit, [], wc, compact_wires=True)
    assert ev(r) == ev(clear) and ev(r)[0] == [True] and "compact" in einfo
    wrong = list(exp)
    wrong[3] ^= 1
    r = stream.evaluate_streaming_pieces(lambda: bristol.iter_device(text, 4096, wrong), wit, [], wc, compact_wires=True)
    wprog = bristol.parse(text, wrong)[0]
    clear = stream.evaluate_streaming(wprog, wit, [], wc, compact_wires=True)
    assert ev(r) == ev(clear) and ev(r)[0] == [False]


def test_program_file_in_windows_to_a_streamed_proof(rv, rule_seeds):
    from reverie_amd import compact, program_file, stream

    prog, w2, w64, wc = circuits.random_mixed(np.random.default_rng(104))
    data = program_file.dumps(prog)
    want = bytes(rv.Proof.new(prog, w2, w64, wc, seeds=rule_seeds))

    def pieces():
        return program_file.iter_device(data, 1000)

    new_wc, pieces2, cinfo = compact.compact_pieces(pieces, wc)
    _, records, info = sweep(prog, wc)
    assert cinfo["compactor"]["scans"] == 2 and cinfo["compactor"]["b2a"] == 1 and new_wc == (info["z64_wires"], info["gf2_wires"])
    for _ in range(2):  # (the second call rewinds)
        assert b"".join(ops.cpu().numpy().tobytes() for ops, _ in pieces2()) == records
    # the caller's compacted pieces through the prover (two passes) and the verifier: the compactor stays the caller's
    proof, got = stream.prove_streaming_pieces(pieces2, w2, w64, new_wc, seeds=rule_seeds)
    assert bytes(proof) == want and "compact" not in got
    assert stream.verify_streaming_pieces(pieces2, new_wc, want)[0]
    assert pieces2.compactor.get_info()["total_ops"] == len(prog)
    assert b"".join(ops.cpu().numpy().tobytes() for ops, _ in pieces2()) == records
    pieces2.compactor.close()
    proof, got = stream.prove_streaming_pieces(pieces, w2, w64, wc, seeds=rule_seeds, compact_wires=True)
    assert bytes(proof) == want and got["compact"]["compactor"]["scans"] == 2
    _, whole = same_pieces_of_the_whole_list(stream, prog, wc, pieces, w2, w64, rule_seeds)
    assert got["wire_store_bytes"] == whole["wire_store_bytes"] and got["chunks"] == whole["chunks"]
    assert stream.verify_streaming_pieces(pieces, wc, want, compact_wires=True)[0]
    # (the list has Random ops: no cleartext evaluation -- both ways answer that)
    assert evaluation(rv, lambda: stream.evaluate_streaming_pieces(pieces, w2, w64, wc, compact_wires=True)) == \
        evaluation(rv, lambda: stream.evaluate_streaming(prog, w2, w64, wc, compact_wires=True)) == ("refused", 8)
