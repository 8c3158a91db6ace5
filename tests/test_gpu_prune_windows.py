"""rv_pruner_* (the kernels of csrc/prune_win.hip) against rv_ops_prune on the whole list: records, old_index and info
byte for byte, through ctypes with every call answering its code, for every way of cutting the mark pass and the emit pass; what
crosses a window border; the order of the calls and the identity of the list; the fall-back; the memory; then what it is for: a
linked list pruned in windows and proved, verified, and the command line."""
import ctypes as C

import numpy as np
import pytest

import prune_cases as pc
import prune_ref
from reverie_amd.ops import B2A, GF2, OP_DTYPE, Z64, SizeHint, program

pytestmark = pytest.mark.gpu

OP_BYTES = OP_DTYPE.itemsize
PAD = 88  # bytes behind the capacity in the output tensors (at least 64, and no multiple of the record size)
OLD_PAD = 16
A5 = 0xA5A5A5A5
CORPUS = pc.corpus()
SMALL = [c for c in CORPUS if len(c[1]) <= 6000]
ERRORS = pc.error_cases()
ARG = prune_ref.ARG


@pytest.fixture(scope="module")
def rv():
    import reverie_amd

    reverie_amd.Context.default()
    return reverie_amd


def on_device(prog):
    import torch

    return torch.from_numpy(np.ascontiguousarray(prog).view(np.uint8).reshape(-1, OP_BYTES).copy()).cuda()


def windows(n, cuts):
    """[lo, hi) of the windows the cut positions make of n ops (a cut that repeats makes an empty window)"""
    b = [0] + list(cuts) + [n]
    return [(b[k], b[k + 1]) for k in range(len(b) - 1)]


class Pruner:
    """rv_pruner through ctypes: every call answers its code; feeds are taken from host and device memory alternately"""

    def __init__(self, rv, wc, og=(), oz=()):
        from reverie_amd import _lib

        self.L = _lib.lib()
        self.lib = _lib
        g, z = np.asarray(og, np.uint32), np.asarray(oz, np.uint32)
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
        self.h = C.c_void_p()
        self.rc = self.L.rv_pruner_begin(rv.Context.default().handle, int(wc[0]), int(wc[1]), p(g), g.size, p(z), z.size, C.byref(self.h))
        self.turn = 0

    def _src(self, ops):
        """-> (pointer, on device, what keeps the memory alive)"""
        ops = np.ascontiguousarray(ops)
        self.turn += 1
        if not len(ops):
            return None, self.turn & 1, ops
        if self.turn & 1:
            t = on_device(ops)
            return C.c_void_p(t.data_ptr()), 1, t
        return ops.ctypes.data_as(C.c_void_p), 0, ops

    def scan(self, ops):
        p, dev, _keep = self._src(ops)
        return self.L.rv_pruner_scan(self.h, p, len(ops), dev)

    def scan_end(self):
        return self.L.rv_pruner_scan_end(self.h)

    def mark(self, ops):
        p, dev, _keep = self._src(ops)
        kept = C.c_size_t(12345)
        return self.L.rv_pruner_mark(self.h, p, len(ops), dev, C.byref(kept)), int(kept.value)

    def mark_end(self):
        pi = self.lib.PruneInfo()
        rc = self.L.rv_pruner_mark_end(self.h, C.byref(pi))
        return rc, {k: int(getattr(pi, k)) for k, _ in pi._fields_}

    def feed(self, ops, cap=None, last_of_wrong_pass=False):
        """-> (code, n_out, the kept records' bytes, old_index); the room is filled with 0xA5, longer than the capacity, and everything
        behind the kept records is checked untouched -- after a code, the whole room (last_of_wrong_pass: the feed is written before
        the pass's digest is judged; then only what lies behind the capacity)"""
        import torch

        n = len(ops)
        cap = n if cap is None else cap
        p, dev, keep = self._src(ops)
        dst = torch.full((cap * OP_BYTES + PAD,), 0xA5, dtype=torch.uint8, device="cuda")
        old = torch.full((cap + OLD_PAD,), -1515870811, dtype=torch.int32, device="cuda")  # 0xA5A5A5A5
        torch.cuda.synchronize()
        n_out = C.c_size_t(12345)
        rc = self.L.rv_pruner_feed(self.h, p, n, dev, C.c_void_p(dst.data_ptr()) if n else None, cap, C.byref(n_out), C.c_void_p(old.data_ptr()) if n else None)
        got, got_old = dst.cpu().numpy(), old.cpu().numpy().view(np.uint32)
        k = int(n_out.value) if rc == 0 else cap if last_of_wrong_pass else 0
        assert k <= cap
        assert (got[k * OP_BYTES:] == 0xA5).all() and (got_old[k:] == A5).all()
        if dev and n:
            assert keep.cpu().numpy().tobytes() == np.ascontiguousarray(ops).tobytes()  # the input is read only
        return rc, int(n_out.value), got[:k * OP_BYTES].tobytes(), got_old[:k].copy()

    def rewind(self):
        return self.L.rv_pruner_rewind(self.h)

    def info(self):
        pi = self.lib.PrunerInfo()
        rc = self.L.rv_pruner_get_info(self.h, C.byref(pi))
        return rc, {k: int(getattr(pi, k)) for k, _ in pi._fields_}

    def close(self):
        if self.h:
            self.L.rv_pruner_destroy(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def emit_pass(pr, ops, cuts):
    """one emit pass -> (records bytes, old_index); every feed answers RV_OK"""
    out, old = [], []
    for lo, hi in windows(len(ops), cuts):
        rc, n_out, rec, idx = pr.feed(ops[lo:hi])
        assert rc == 0 and n_out * OP_BYTES == len(rec), (lo, hi, rc)
        out.append(rec)
        old.append(idx)
    return b"".join(out), np.concatenate(old) if old else np.zeros(0, np.uint32)


def run(rv, case, scan_cuts, mark_cuts, emit_cuts):
    """the three passes -> (rv_prune_info, rv_pruner_info), the records and old_index checked against rv_ops_prune's"""
    name, ops, wc, og, oz = case
    want, winfo, wold = rv.prune_ops(ops, wc, og, oz)
    n = len(ops)
    with Pruner(rv, wc, og, oz) as pr:
        assert pr.rc == 0
        for lo, hi in windows(n, scan_cuts):
            assert pr.scan(ops[lo:hi]) == 0
        assert pr.scan_end() == 0
        kept = 0
        for lo, hi in reversed(windows(n, mark_cuts)):
            rc, here = pr.mark(ops[lo:hi])
            assert rc == 0, (name, lo, hi, rc)
            kept += here
        rc, info = pr.mark_end()
        assert rc == 0 and kept == winfo["n_kept"], name
        skip = ("device_rounds", "on_device")
        assert {k: v for k, v in info.items() if k not in skip} == {k: v for k, v in winfo.items() if k not in skip}, (name, mark_cuts)
        rec, old = emit_pass(pr, ops, emit_cuts)
        assert rec == want.tobytes() and (old == wold).all(), (name, mark_cuts, emit_cuts)
        rc, pinfo = pr.info()
        assert rc == 0 and pinfo["total_ops"] == n and pinfo["n_kept"] == len(want)
    return info, pinfo


def cuttings(n):
    """the issue's cuttings of a list of n ops (those that fit it)"""
    out = [[]]
    if n >= 2:
        out.append(sorted({1, n - 1}))
    for group in ((256,), (255, 257), (2047, 2049)):
        if n > group[-1]:
            out.append(list(group))
    if n >= 4:
        out.append([n // 2, n // 2])  # an empty feed between two others
    if 1 < n <= 14:
        out.append(list(range(1, n)))
    return out


@pytest.mark.parametrize("case", SMALL, ids=[c[0] for c in SMALL])
def test_cuts(rv, case):
    """every cutting of the mark pass, each with another cutting of the emit pass (and of the scan)"""
    name, ops, wc, og, oz = case
    cs = cuttings(len(ops))
    layers = prune_ref.peel(ops, og, oz)[1]["device_rounds"]
    for k, mark in enumerate(cs):
        info, _ = run(rv, case, cs[(k + 2) % len(cs)], mark, cs[(k + 1) % len(cs)])
        assert info["on_device"] == 1
        if not mark:
            assert info["device_rounds"] == layers, name  # one feed that holds the whole list: rv_ops_prune_device's figure


@pytest.mark.parametrize("name", ["length_70000", "dead_layer_70000"])
def test_cuts_of_long_lists(rv, name):
    case = {c[0]: c for c in CORPUS}[name]
    n = len(case[1])
    for scan, mark, emit in (([], [], [n // 2]), ([n // 3], [2047, 2049, 40000], [255, 257, 65536]), ([1], [1, n - 1], [])):
        run(rv, case, scan, mark, emit)


def _crossings():
    G = GF2
    out = []
    add = lambda name, ops, wc, cuts, og=(), oz=(): out.append((name, program(ops), wc, list(og), list(oz), cuts))
    add("live_reader_behind_the_border", [G.Input(0), G.AddConst(1, 0, 1), G.AssertZero(1)], (0, 2), [2])
    add("dead_reader_behind_the_border", [G.Input(0), G.AddConst(1, 0, 1), G.Mul(2, 1, 1)], (0, 3), [2])
    add("dead_chain_through_three_windows", [G.Input(0), G.AddConst(1, 0, 1), G.AddConst(2, 1, 1), G.AddConst(3, 2, 1), G.AddConst(4, 3, 1), G.AssertZero(0)],
        (0, 5), [2, 4])
    add("needed_index_written_twice", [G.Input(0), G.AddConst(1, 0, 1), G.AddConst(1, 0, 0), G.AssertZero(1)], (0, 2), [1, 3])
    add("kill_then_gen", [G.Input(0), G.AddConst(5, 0, 1), G.AssertZero(5), G.AddConst(5, 0, 0), G.AssertZero(5)], (0, 6), [2, 4])
    add("kill_then_gen_reader_dead", [G.Input(0), G.AddConst(5, 0, 1), G.Mul(6, 5, 5), G.AddConst(5, 0, 0), G.AssertZero(5)], (0, 7), [2, 4])
    add("output_written_in_the_first_window", [G.Const(3, 1), G.Input(0), G.Mul(1, 0, 0), G.Mul(2, 0, 0)], (0, 4), [2, 3], og=[3])
    add("output_nobody_writes", [G.Input(0), G.Mul(1, 0, 0), Z64.Const(0, 1)], (4, 12), [1, 2], og=[9, 1], oz=[3])
    b2a = [G.Input(0)] + [G.AddConst(10 + i, 0, i & 1) for i in range(64)] + [G.AddConst(100 + i, 0, 1) for i in range(64)]
    b2a += [B2A(0, 10), B2A(1, 100), Z64.AssertZero(0)]
    add("b2a_sources_in_two_earlier_windows", b2a, (2, 164), [1 + 30, 1 + 64 + 30, 1 + 128])
    add("sizehint_grows_both_counts", [G.Input(0), G.Mul(1, 0, 0), SizeHint(4, 80), G.Const(70, 1), B2A(3, 16), Z64.AssertZero(3), G.AssertZero(70)],
        (0, 2), [2, 4])
    add("input_read_two_windows_on", [G.Input(0), G.Input(1), G.Const(2, 1), G.Add(3, 1, 2), G.AssertZero(3), Z64.Input(0)], (1, 4), [2, 3])
    add("both_domains", [G.Input(0), Z64.Input(0), G.Mul(1, 0, 0), Z64.Mul(1, 0, 0), Z64.Mul(2, 1, 1), G.AssertZero(1), Z64.Add(3, 1, 0), Z64.AssertZero(3),
                         G.Random(2), Z64.Random(4)], (5, 3), [3, 6])
    return out


CROSSINGS = _crossings()


@pytest.mark.parametrize("case", CROSSINGS, ids=[c[0] for c in CROSSINGS])
def test_what_crosses_a_border(rv, case):
    name, ops, wc, og, oz, cuts = case
    want, winfo, _ = rv.prune_ops(ops, wc, og, oz)
    info, _ = run(rv, case[:5], [], cuts, cuts)
    run(rv, case[:5], cuts, cuts, [])
    run(rv, case[:5], [], list(range(1, len(ops))), list(range(1, len(ops))))
    expect = {"dead_reader_behind_the_border": 1, "dead_chain_through_three_windows": 2, "kill_then_gen": 5, "kill_then_gen_reader_dead": 3,
              "needed_index_written_twice": 3, "live_reader_behind_the_border": 3, "output_written_in_the_first_window": 2}
    if name in expect:  # (the lists do what their names say)
        assert winfo["n_kept"] == expect[name], name
    if name == "b2a_sources_in_two_earlier_windows":
        assert winfo["dropped_b2a"] == 1 and winfo["n_kept"] == 1 + 64 + 2
    if name == "input_read_two_windows_on":
        assert winfo["unread_gf2_inputs"] == 1 and winfo["unread_z64_inputs"] == 1 and winfo["n_dropped"] == 0


def test_order_of_calls(rv):
    """every call out of order is RV_E_ARG and changes nothing: the passes go on to the right bytes afterwards"""
    name, ops, wc, og, oz = {c[0]: c for c in CORPUS}["length_2049"]
    want, winfo, wold = rv.prune_ops(ops, wc, og, oz)
    n = len(ops)
    with Pruner(rv, wc, og, oz) as pr:
        assert pr.mark(ops[:5])[0] == ARG and pr.mark_end()[0] == ARG and pr.feed(ops[:5])[0] == ARG and pr.rewind() == ARG
        assert pr.scan(ops[:1000]) == 0
        assert pr.mark(ops[:5])[0] == ARG and pr.feed(ops[:5])[0] == ARG
        assert pr.info()[1]["total_ops"] == 1000
        assert pr.scan(ops[1000:]) == 0 and pr.scan_end() == 0
        assert pr.scan(ops[:5]) == ARG and pr.scan_end() == ARG and pr.feed(ops[:5])[0] == ARG and pr.rewind() == ARG
        assert pr.mark_end()[0] == ARG  # (nothing marked yet: the pass stopped short of ordinal 0)
        assert pr.mark(ops[1500:]) == (0, int(np.count_nonzero(np.isin(np.arange(1500, n), wold))))
        assert pr.mark(ops[:1501])[0] == ARG  # more than what is left
        assert pr.mark_end()[0] == ARG and pr.scan(ops[:5]) == ARG
        assert pr.mark(ops[:1500])[0] == 0
        assert pr.mark(ops[:1])[0] == ARG and pr.mark(ops[:0])[0] == 0
        rc, info = pr.mark_end()
        assert rc == 0 and info["n_kept"] == len(want)
        assert pr.mark(ops[:0])[0] == ARG and pr.mark_end()[0] == ARG and pr.scan_end() == ARG
        first = pr.feed(ops[:700])
        assert first[0] == 0
        assert pr.rewind() == ARG  # after a short pass
        assert pr.feed(ops[700:], cap=0)[0] == ARG  # room below the kept count: nothing written (the helper checks), nothing moved
        assert pr.feed(ops[699:])[0] == ARG         # more than what is left
        rest = pr.feed(ops[700:])
        assert rest[0] == 0 and first[2] + rest[2] == want.tobytes() and (np.concatenate([first[3], rest[3]]) == wold).all()
        assert pr.feed(ops[:1])[0] == ARG and pr.feed(ops[:0])[0] == 0
        # two full emit passes, cut differently, give the same bytes
        assert pr.rewind() == 0
        rec, old = emit_pass(pr, ops, [1, 255, 256, 256, 2048])
        assert rec == want.tobytes() and (old == wold).all()
        assert pr.rewind() == 0
        rec, old = emit_pass(pr, ops, [])
        assert rec == want.tobytes() and (old == wold).all()


def test_overlap_and_pointers(rv):
    """any overlap of d_out with a device feed, host memory as d_out, a feed called device that is not: RV_E_ARG before a launch"""
    import torch

    name, ops, wc, og, oz = {c[0]: c for c in CORPUS}["length_257"]
    n = len(ops)
    with Pruner(rv, wc, og, oz) as pr:
        assert pr.scan(ops) == 0 and pr.scan_end() == 0 and pr.mark(ops)[0] == 0 and pr.mark_end()[0] == 0
        src = torch.full((2 * n * OP_BYTES,), 0xA5, dtype=torch.uint8, device="cuda")
        src[:n * OP_BYTES] = on_device(ops).reshape(-1)
        torch.cuda.synchronize()
        p = src.data_ptr()
        f = pr.L.rv_pruner_feed
        n_out = C.c_size_t(0)
        for d_out in (p, p + OP_BYTES, p + (n - 1) * OP_BYTES):
            assert f(pr.h, C.c_void_p(p), n, 1, C.c_void_p(d_out), n, C.byref(n_out), None) == ARG
        assert f(pr.h, C.c_void_p(p), n, 1, C.c_void_p(p + n * OP_BYTES + 4), n - 1, C.byref(n_out), None) == ARG  # misaligned
        hostmem = ops.copy()
        assert f(pr.h, C.c_void_p(p), n, 1, C.c_void_p(hostmem.ctypes.data), n, C.byref(n_out), None) == ARG
        assert f(pr.h, C.c_void_p(hostmem.ctypes.data), n, 1, C.c_void_p(p + n * OP_BYTES), n, C.byref(n_out), None) == ARG
        assert f(pr.h, C.c_void_p(p), n, 1, None, n, C.byref(n_out), None) == ARG
        assert src.cpu().numpy()[n * OP_BYTES:].tobytes() == b"\xA5" * (n * OP_BYTES) and hostmem.tobytes() == ops.tobytes()
        assert f(pr.h, C.c_void_p(p), n, 1, C.c_void_p(p + n * OP_BYTES), n, C.byref(n_out), None) == 0  # right behind the feed is no overlap
        want = rv.prune_ops(ops, wc, og, oz)[0]
        k = int(n_out.value)
        assert src.cpu().numpy()[n * OP_BYTES:(n + k) * OP_BYTES].tobytes() == want.tobytes()


def test_not_the_scanned_list(rv):
    name, ops, wc, og, oz = {c[0]: c for c in CORPUS}["length_2049"]
    n = len(ops)
    full = prune_ref.check  # (the list is valid)
    assert full(ops, wc, og, oz) == 0
    k = int(np.flatnonzero((ops["domain"] == 0) & (ops["opcode"] == 6))[-1])  # a GF(2) Mul
    final_g = max(int(wc[1]), int(ops["b"][ops["domain"] == 3].max(initial=0)))
    # an index at or above the final count: RV_E_ARG at the feed that holds the record, and nothing is addressed by it
    bad = ops.copy()
    bad["a"][k] = final_g
    with Pruner(rv, wc, og, oz) as pr:
        assert pr.scan(ops) == 0 and pr.scan_end() == 0
        lo = (k // 700) * 700
        for a, b in reversed(windows(n, [700, 1400])):
            rc, _ = pr.mark(bad[a:b])
            assert rc == (ARG if a == lo else 0)
            if rc:
                break
        assert pr.mark(ops[lo:b])[0] == 0  # the feed of the scanned list goes through afterwards
    # a changed imm: every index is fine, the digest is not -- RV_E_ARG at mark_end
    bad = ops.copy()
    bad["imm"][k] ^= 1
    with Pruner(rv, wc, og, oz) as pr:
        assert pr.scan(ops) == 0 and pr.scan_end() == 0
        for a, b in reversed(windows(n, [700, 1400])):
            assert pr.mark(bad[a:b])[0] == 0
        assert pr.mark_end()[0] == ARG
    # an emit pass with two records swapped: RV_E_ARG at its last feed
    bad = ops.copy()
    bad[[10, 11]] = bad[[11, 10]]
    assert bad[10].tobytes() != ops[10].tobytes()
    with Pruner(rv, wc, og, oz) as pr:
        assert pr.scan(ops) == 0 and pr.scan_end() == 0 and pr.mark(ops)[0] == 0 and pr.mark_end()[0] == 0
        assert pr.feed(bad[:1000])[0] == 0 and pr.feed(bad[1000:2000])[0] == 0
        assert pr.feed(bad[2000:], last_of_wrong_pass=True)[0] == ARG


@pytest.mark.parametrize("case", ERRORS, ids=[c[0] for c in ERRORS])
def test_error_lists(rv, case):
    """rv_ops_prune's code, answered by the scan feed that holds the first bad op, or by scan_end for an output out of range; only
    destroy is accepted afterwards"""
    name, ops, wc, og, oz, _ = case
    want = prune_ref.check(ops, wc, og, oz)
    with pytest.raises(rv.ReverieError) as e:
        rv.prune_ops(ops, wc, og, oz)
    assert e.value.code == want != 0
    n = len(ops)
    first_bad = None
    if prune_ref.check(ops, wc):  # (the shortest prefix the validation refuses ends on the first bad op)
        lo, hi = 0, n
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if prune_ref.check(ops[:mid], wc) else (mid, hi)
        first_bad = hi - 1
    step = max(1, n // 3)
    with Pruner(rv, wc, og, oz) as pr:
        for lo in range(0, n, step):
            rc = pr.scan(ops[lo:lo + step])
            if first_bad is not None and lo <= first_bad < lo + step:
                assert rc == want, name
                break
            assert rc == 0, name
        else:
            assert first_bad is None and pr.scan_end() == want == ARG, name
        assert pr.scan(ops[:1]) == ARG and pr.scan_end() == ARG and pr.mark(ops[:1])[0] == ARG and pr.info()[0] == ARG


def test_fallback(rv, monkeypatch):
    """RV_PRUNE_MAX_ROUNDS=64: the window that holds the depth-5 000 chain's tail is stepped on the host; the same bytes"""
    case = {c[0]: c for c in CORPUS}["dead_chain_5000"]
    monkeypatch.setenv("RV_PRUNE_MAX_ROUNDS", "64")
    info, pinfo = run(rv, case, [], [2500], [100])
    assert info["on_device"] == 0 and pinfo["host_feeds"] >= 1 and pinfo["mark_feeds"] == 2 and info["device_rounds"] >= 64
    monkeypatch.delenv("RV_PRUNE_MAX_ROUNDS")
    info, pinfo = run(rv, case, [], [2500], [100])
    assert info["on_device"] == 1 and pinfo["host_feeds"] == 0 and info["device_rounds"] == 5000


def test_memory(rv):
    """what is held between calls is a byte per wire index and per op and the words; a call's work memory follows the feed"""
    case = {c[0]: c for c in CORPUS}["length_70000"]
    name, ops, wc, og, oz = case
    n = len(ops)
    final = [max(int(wc[0]), int(ops["a"][ops["domain"] == 3].max(initial=0))), max(int(wc[1]), int(ops["b"][ops["domain"] == 3].max(initial=0)))]
    small = list(range(2048, n, 2048))
    _, one = run(rv, case, [], [], [])
    _, many = run(rv, case, small, small, small)
    for pinfo in (one, many):
        assert pinfo["state_bytes"] <= sum(final) + n + 4096
    assert many["mark_feeds"] == len(small) + 1 and one["mark_feeds"] == 1
    # a whole-list call takes 33 to 49 bytes per op, a host feed 24 more; the sort's histograms and the scans' sums are a few KiB
    assert one["peak_feed_bytes"] >= 33 * n
    assert many["peak_feed_bytes"] <= 2048 * (49 + 24) + 65536
    assert many["peak_feed_bytes"] * 8 < one["peak_feed_bytes"]


# ---- what it is for ----
def _half_asserted_adders(device):
    """four chained 64-bit adders of which the tail asserts the low 32 sum bits: the upper half of the last adder is dead"""
    import link_cases as lc

    nl, _, tail, bits, total = lc.adder_chain(n=4, device=device)
    nl.set_tail(tail(total)[:64])
    return nl, np.asarray(bits, np.uint8)


def test_prove_and_verify_from_a_linked_list(rv, oracle, rule_seeds):
    """LinkPlan.pieces -> prune_pieces -> prove_streaming_pieces(compact_wires=True) is byte for byte the oracle's proof of
    rv_ops_prune's list; verify_streaming_pieces(prune=True) accepts it; the unpruned stream's proof is longer"""
    from reverie_amd import prune, stream

    nl_host, wit = _half_asserted_adders(False)
    ops, info = nl_host.link_host()
    wc = info["wire_counts"]
    pruned, pinfo, _ = rv.prune_ops(ops, wc)
    assert pinfo["dropped_gf2_mul"] > 0
    want = oracle.prove(pruned, wit.tolist(), [], wc, rule_seeds, threads=2)
    nl, _ = _half_asserted_adders(True)
    with nl.plan() as plan:
        pieces = plan.pieces(300)
        assert [t.cpu().numpy().tobytes() for t, _ in pieces.backwards()] == [t.cpu().numpy().tobytes() for t, _ in pieces()][::-1]
        pieces2, winfo = prune.prune_pieces(pieces, wc)
        try:
            assert {k: v for k, v in winfo.items() if k not in ("device_rounds", "on_device", "pruner")} == \
                {k: v for k, v in pinfo.items() if k not in ("device_rounds", "on_device")}
            assert winfo["pruner"]["total_ops"] == len(ops) and winfo["pruner"]["host_feeds"] == 0
            got = b"".join(t.cpu().numpy().tobytes() for t, _ in pieces2())
            assert got == pruned.tobytes()
            assert tuple(map(sum, zip(*(c for _, c in pieces2())))) == (info["n_input_gf2"], info["n_input_z64"])
            proof, sinfo = stream.prove_streaming_pieces(pieces2, wit, [], wc, seeds=rule_seeds, compact_wires=True)
            assert bytes(proof) == want and "compact" in sinfo
        finally:
            pieces2.pruner.close()
        # prune=True: the same, made inside the call; prover and verifier both prune
        proof2, sinfo = stream.prove_streaming_pieces(pieces, wit, [], wc, seeds=rule_seeds, compact_wires=True, prune=True)
        assert bytes(proof2) == want and sinfo["prune"]["n_kept"] == len(pruned) and "compact" in sinfo
        ok, vinfo = stream.verify_streaming_pieces(pieces, wc, want, prune=True)
        assert ok and vinfo["prune"]["n_dropped"] == pinfo["n_dropped"]
        plain, plain_info = stream.prove_streaming_pieces(pieces, wit, [], wc, seeds=rule_seeds)
        assert "prune" not in plain_info and len(bytes(plain)) > len(want)
        ev_info = {}
        assert stream.evaluate_streaming_pieces(pieces, wit, [], wc, prune=True, info=ev_info).n_failed.tolist() == [0]
        assert ev_info["prune"]["n_kept"] == len(pruned)


def test_window_pieces_on_a_tensor_and_a_memmap(rv, tmp_path):
    import torch

    from reverie_amd import prune

    name, ops, wc, og, oz = {c[0]: c for c in CORPUS}["length_2049"]
    want, winfo, _ = rv.prune_ops(ops, wc, og, oz)
    path = str(tmp_path / "p.rvops")
    ops.tofile(path)
    for src, w in ((on_device(ops), 500), (np.memmap(path, dtype=OP_DTYPE, mode="r", shape=(len(ops),)), 256), (on_device(ops).reshape(-1), 4096),
                   (on_device(ops).view(torch.int64), 1000)):
        pieces2, info = prune.prune_pieces(prune.window_pieces(src, w), wc, og, oz)
        try:
            for _ in range(2):  # (the second pass rewinds)
                assert b"".join(t.cpu().numpy().tobytes() for t, _ in pieces2()) == want.tobytes()
            assert info["n_kept"] == len(want) and info["pruner"]["mark_feeds"] == -(-len(ops) // w)
        finally:
            pieces2.pruner.close()
    # other cuts for the backward pass than for the forward ones
    fwd, bwd = prune.window_pieces(ops, 300), prune.window_pieces(ops, 777).backwards
    pieces2, info = prune.prune_pieces(fwd, wc, og, oz, backwards=bwd)
    assert b"".join(t.cpu().numpy().tobytes() for t, _ in pieces2()) == want.tobytes()
    pieces2.pruner.close()


def test_command_line(rv, tmp_path, capfd, monkeypatch, rule_seeds):
    """--prune-windows --compact-windows on an rvops file gives --prune --compact-wires' proof bytes (the command line draws its seeds
    at random: both runs are handed the same ones); convert writes --prune's file"""
    import functools

    from reverie_amd import stream
    from reverie_amd.__main__ import main

    monkeypatch.setattr(stream, "prove_streaming_pieces", functools.partial(stream.prove_streaming_pieces, seeds=rule_seeds))

    name, ops, wc, wit_g, _ = pc.proof_programs()[0]
    prog, wit = str(tmp_path / "p.rvops"), str(tmp_path / "w.txt")
    ops.tofile(prog)
    with open(wit, "w") as f:
        f.write("".join(str(b) for b in wit_g) + "\n")
    proofs = {}
    for tag, flags in (("whole", ["--prune", "--compact-wires"]), ("windows", ["--prune-windows", "--compact-windows"])):
        out = str(tmp_path / (tag + ".proof"))
        base = ["--program-path", prog, "--program-format", "rvops", "--stream"]
        assert main(["--operation", "prove", "--witness-path", wit, "--proof-path", out] + base + flags) == 0
        assert "prune: %d ops -> " % len(ops) in capfd.readouterr().err
        assert main(["--operation", "verify", "--proof-path", out] + base + flags) == 0
        proofs[tag] = open(out, "rb").read()
    assert proofs["whole"] == proofs["windows"]
    conv = ["--operation", "convert", "--program-path", prog, "--program-format", "rvops", "--output-format", "rvops"]
    assert main(conv + ["--output-path", str(tmp_path / "a.rvops"), "--prune"]) == 0
    assert main(conv + ["--output-path", str(tmp_path / "b.rvops"), "--prune-windows"]) == 0
    a, b = open(str(tmp_path / "a.rvops"), "rb").read(), open(str(tmp_path / "b.rvops"), "rb").read()
    assert a == b == rv.prune_ops(ops, wc)[0].tobytes()
    assert main(["--operation", "oneshot", "--evaluator", "stream", "--witness-path", wit, "--program-path", prog, "--program-format", "rvops",
                 "--prune-windows"]) == 0
