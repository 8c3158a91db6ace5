"""rv_folder_* (the kernels of csrc/fold_win.hip and fold_dev_kernels.inc) against rv_ops_fold, the host definition: records and
counts byte for byte on the cases of tests/fold_cases.py over the cuttings of tests/fold_window_ref.py, from host and device feeds,
into outputs on both alignments, in place and counting only; window lengths around the tile; layers whose seeds sit in the window
before; one feed against rv_ops_fold_device; rewind; the log and its replays; the fall-back; the codes, the pointer rules and the
order of the calls; then what it is for: proofs, verification and evaluation over folded pieces, and the command line."""
import ctypes as C
import os

import numpy as np
import pytest

import fold_cases as fc
import fold_ref
import fold_window_ref as fw
from reverie_amd.ops import OP_DTYPE

pytestmark = pytest.mark.gpu

OP_BYTES = OP_DTYPE.itemsize
PAD = 88  # bytes behind the list in the output tensors (at least 64, and no multiple of the record size)
CHUNK = 1024
ARG = 9


def _limits():
    from reverie_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    lim = (C.c_uint32 * 5)()
    assert _lib.lib().rv_hook_fold_limits(lim) == 0
    return [int(x) for x in lim]


LIMITS = _limits()
SOLO = LIMITS[1]
CORPUS = fc.corpus(SOLO)
CASES = {c[0]: c for c in CORPUS}
ERRORS = fc.error_cases()
PROOFS = fc.proof_programs()
ONE_OP_FEEDS = ("length_257", f"known_layer_{SOLO + 1}")  # the lists above 64 ops that are also fed op by op
_whole = {}


@pytest.fixture(scope="module")
def rv():
    import reverie_amd

    reverie_amd.Context.default()
    return reverie_amd


def whole(rv, case):
    """rv_ops_fold's (record bytes, info) of a case, computed once"""
    if case[0] not in _whole:
        out, info = rv.fold_ops(case[1], case[2])
        _whole[case[0]] = (out.tobytes(), info)
    return _whole[case[0]]


def launches():
    from reverie_amd import _lib

    out = (C.c_uint64 * 4)()
    assert _lib.lib().rv_hook_fold_launches(out) == 0
    return [int(x) for x in out]


def _dict(s):
    return {k: int(getattr(s, k)) for k, _ in s._fields_}


class Folder:
    """rv_folder through ctypes, on raw pointers"""

    def __init__(self, rv, wc, flags=0):
        from reverie_amd import _lib

        self.L, self.h = _lib.lib(), C.c_void_p()
        self.rc = self.L.rv_folder_begin(rv.Context.default().handle, int(wc[0]), int(wc[1]), flags, C.byref(self.h))

    def feed(self, ops, n, on_device, d_out):
        return self.L.rv_folder_feed(self.h, C.c_void_p(ops) if ops else None, n, on_device, C.c_void_p(d_out) if d_out else None)

    def replay(self, ops, n, on_device, first, d_out):
        return self.L.rv_folder_replay(self.h, C.c_void_p(ops) if ops else None, n, on_device, first, C.c_void_p(d_out) if d_out else None)

    def end(self):
        from reverie_amd import _lib

        fi = _lib.FoldInfo()
        return self.L.rv_folder_end(self.h, C.byref(fi)), _dict(fi)

    def rewind(self):
        return self.L.rv_folder_rewind(self.h)

    def replay_end(self):
        return self.L.rv_folder_replay_end(self.h)

    def info(self):
        from reverie_amd import _lib

        fi = _lib.FolderInfo()
        return self.L.rv_folder_get_info(self.h, C.byref(fi)), _dict(fi)

    def close(self):
        if self.h:
            self.L.rv_folder_destroy(self.h)
            self.h = C.c_void_p()


def windows(n, cuts):
    b = [0] + [int(c) for c in cuts] + [n]
    return list(zip(b, b[1:]))


def buffers(ops, off):
    """-> (raw host bytes, the source tensor with the list `off` bytes in, an output tensor of the same shape, both 0xA5 elsewhere)"""
    import torch

    n = len(ops)
    raw = np.ascontiguousarray(ops).view(np.uint8).reshape(-1)
    src = torch.full((off + n * OP_BYTES + PAD,), 0xA5, dtype=torch.uint8, device="cuda")
    src[off:off + n * OP_BYTES] = torch.from_numpy(raw.copy()).cuda()
    dst = torch.full((off + n * OP_BYTES + PAD,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return raw, src, dst


def run_feeds(rv, ops, wc, cuts, feeds="device", mode="new", off=0, flags=0, folder=None):
    """the list fed window by window -> (rc of the first failing call or 0, record bytes, info, the folder (open)).  feeds "host":
    every window is uploaded from host memory; mode "new": window [lo, hi) goes to d_out + lo records, d_out `off` bytes (a multiple
    of 8) into a tensor filled with 0xA5; "inplace": d_out is the feed; "count": d_out NULL"""
    n = len(ops)
    raw, src, dst = buffers(ops, off)
    host = np.ascontiguousarray(ops)
    f = folder or Folder(rv, wc, flags)
    assert f.rc == 0
    rc = 0
    for lo, hi in windows(n, cuts):
        p = (host.ctypes.data + lo * OP_BYTES) if feeds == "host" else (src.data_ptr() + off + lo * OP_BYTES)
        q = None if mode == "count" else p if mode == "inplace" else dst.data_ptr() + off + lo * OP_BYTES
        rc = f.feed(p if hi > lo else None, hi - lo, 0 if feeds == "host" else 1, q if hi > lo else None)
        if rc:
            break
    rc_end, info = f.end() if rc == 0 else (rc, None)
    got_src, got = src.cpu().numpy(), dst.cpu().numpy()
    assert got_src[:off].tobytes() == b"\xA5" * off and got_src[off + n * OP_BYTES:].tobytes() == b"\xA5" * PAD
    if mode == "inplace":
        got = got_src
    else:
        assert got_src[off:off + n * OP_BYTES].tobytes() == raw.tobytes() and host.tobytes() == raw.tobytes()  # the input is read only
        assert got[:off].tobytes() == b"\xA5" * off and got[off + n * OP_BYTES:].tobytes() == b"\xA5" * PAD
    return rc or rc_end, got[off:off + n * OP_BYTES].tobytes(), info, f


def check(rv, case, cuts, label="", **kw):
    name, ops, wc = case
    want, winfo = whole(rv, case)
    rc, out, info, f = run_feeds(rv, ops, wc, cuts, **kw)
    try:
        assert rc == 0, (name, label, rc)
        assert out == (b"\xA5" * len(out) if kw.get("mode") == "count" else want), (name, label, cuts)
        assert {k: v for k, v in info.items() if k != "device_rounds"} == dict({k: v for k, v in winfo.items() if k != "device_rounds"}, on_device=1), (name, label)
        rc, fi = f.info()
        assert rc == 0 and fi["total_ops"] == len(ops) and fi["host_feeds"] == 0 and fi["feeds"] == sum(hi > lo for lo, hi in windows(len(ops), cuts))
        assert fi["log_records"] == (winfo["n_rewritten"] if kw.get("flags") else 0)
    finally:
        f.close()
    return info


def case_cuttings(case, k):
    out = []
    for label, cuts in fw.cuttings(len(case[1]), np.random.default_rng(8000 + k), every_single=64):
        if label == "one_op_feeds" and len(case[1]) > 64 and case[0] not in ONE_OP_FEEDS:
            continue
        out.append((label, cuts))
    return out


@pytest.mark.parametrize("k", range(len(CORPUS)), ids=[c[0] for c in CORPUS])
def test_device_equals_host(rv, k):
    """device feeds into a 16-byte aligned output; the feed modes take turns over the cuttings: host feeds, an output 8 bytes off
    (a window's records then begin on either alignment, at odd record offsets), in place, counting only with the log"""
    case = CORPUS[k]
    variants = ({}, {"feeds": "host"}, {"off": 8}, {"mode": "inplace", "off": 8 * (len(case[1]) & 1)}, {"mode": "count", "flags": 1},
                {"feeds": "host", "off": 8, "flags": 1})
    for j, (label, cuts) in enumerate(case_cuttings(case, k)):
        check(rv, case, cuts, label)
        if label == "one_op_feeds" and len(case[1]) > 300:  # (thousands of feeds: once)
            continue
        if j % 2 == 0 or label in ("whole", "one_op_feeds", "empty_ends_doubled"):
            check(rv, case, cuts, label, **variants[1 + (j // 2) % 5])


def test_every_mode_on_one_list(rv):
    case = CASES["length_513"]
    for cuts in ([], [1, 256, 257], [200, 200, 511]):
        for feeds in ("host", "device"):
            for mode in ("new", "count") + (("inplace",) if feeds == "device" else ()):
                for off in (0, 8):
                    check(rv, case, cuts, feeds=feeds, mode=mode, off=off, flags=1)


def test_window_lengths(rv):
    """windows of 255, 256, 257 and 513 records over the length_* lists: a window's last tile is short, whole, one record long"""
    for name in ("length_255", "length_256", "length_257", "length_513"):
        case = CASES[name]
        n = len(case[1])
        for w in (255, 256, 257, 513):
            for off in (0, 8):
                check(rv, case, list(range(w, n, w)), f"window_{w}", off=off)
    # and a longer list, so that several whole windows of each length pass
    ops, wc = fc.of_length(2000, 31)
    case = ("length_2000", ops, wc)
    for w in (255, 256, 257, 513):
        check(rv, case, list(range(w, 2000, w)), f"window_{w}", flags=1)


def test_solo_limit_layers_seeded_from_the_tables(rv):
    """known_layer_W: the Const that seeds the layer sits in the window before it, so the whole frontier of W ops comes from the
    tables, at once; W around the solo limit"""
    for w in (SOLO - 1, SOLO, SOLO + 1):
        case = CASES[f"known_layer_{w}"]
        want, winfo = whole(rv, case)
        info = check(rv, case, [2], "consts_in_previous_window")
        # window 1: the Const alone, one layer; window 2: the W AddConsts are known at once, one layer, and their readers hear nothing new
        assert info["device_rounds"] == 2 and info["n_known"] == w + 1
        check(rv, case, [2, 2 + w], "three_windows", mode="inplace")
        check(rv, case, [1, 2], "input_const_rest", feeds="host", flags=1)


def test_single_feed_is_the_whole_list_call(rv):
    """one feed that holds the whole list: rv_ops_fold_device's info, device_rounds included; and the whole-list call itself launches
    what it launched before there were windows (the figures of tests/test_gpu_fold.py)"""
    import torch

    from reverie_amd import _lib

    for name in ("nothing_known", "known_chain_65", f"known_layer_{SOLO}", f"known_layer_{SOLO + 1}", "widen_past_solo_and_narrow", "length_513",
                 "unwritten_reads", "b2a_64_known", "sizehint_grows"):
        case = CASES[name]
        _, ops, wc = case
        want, winfo = whole(rv, case)
        t = torch.from_numpy(np.ascontiguousarray(ops).view(np.uint8).reshape(-1, OP_BYTES).copy()).cuda()
        before = launches()
        d_out, dinfo = rv.fold_ops(t, wc)
        after = launches()
        assert d_out.cpu().numpy().tobytes() == want
        widths = fold_ref.layers(ops)[1]
        assert dinfo == dict(winfo, device_rounds=len(widths), on_device=1)
        assert after[3] == before[3] and (after[2] > before[2]) == bool(widths), name
        if name == "nothing_known":
            assert after == before  # (copied: no rewrite launch either)
        else:
            assert (after[0] - before[0], after[1] - before[1]) == (1, 0), name
        if name in (f"known_layer_{SOLO}", f"known_layer_{SOLO + 1}"):
            assert after[2] - before[2] == 2 * LIMITS[2], name  # one interval: a solo and a wide launch per iteration
        delta = [a - b for a, b in zip(after, before)]
        before = launches()
        rc, out, info, f = run_feeds(rv, ops, wc, [])
        f.close()
        assert rc == 0 and out == want and info == dinfo, name
        # (the single feed launches what the whole-list call launched)
        assert [a - b for a, b in zip(launches(), before)] == delta, name


def test_rewind(rv):
    """the second pass gives the same bytes and counts; a second pass over an altered list answers RV_E_ARG at its last feed"""
    case = CASES["length_513"]
    name, ops, wc = case
    want, winfo = whole(rv, case)
    rc, out, info, f = run_feeds(rv, ops, wc, [100, 300], flags=1)
    try:
        assert rc == 0 and out == want
        assert f.info()[1]["log_records"] == winfo["n_rewritten"]
        assert f.rewind() == 0
        rc, out2, info2, _ = run_feeds(rv, ops, wc, [7, 256, 400, 512], feeds="host", off=8, folder=f)
        assert rc == 0 and out2 == want and info2 == dict(info, device_rounds=info2["device_rounds"])
        assert f.info()[1]["log_records"] == winfo["n_rewritten"] and f.info()[1]["total_ops"] == 513
        # altered: one record's imm
        assert f.rewind() == 0
        other = ops.copy()
        other["imm"][500] ^= 1
        rc, _, _, _ = run_feeds(rv, other, wc, [100, 300], folder=f)
        assert rc == ARG
        # a pass that stops short cannot be ended; more ops than the list had are refused
        assert f.end()[0] == ARG
    finally:
        f.close()
    rc, _, _, f = run_feeds(rv, ops, wc, [100])
    try:
        assert rc == 0 and f.rewind() == 0
        host = np.ascontiguousarray(ops)
        assert f.feed(host.ctypes.data, 512, 0, None) == 0 and f.end()[0] == ARG
        assert f.feed(host.ctypes.data, 2, 0, None) == ARG  # beyond the list
        assert f.feed(host.ctypes.data + 512 * OP_BYTES, 1, 0, None) == 0 and f.end()[0] == 0
    finally:
        f.close()


def replay_all(rv, f, ops, order, cuts, feeds="device", inplace=False, off=0):
    """the windows of `cuts` replayed in `order` -> (rc of the first failing call or 0, the bytes)"""
    n = len(ops)
    raw, src, dst = buffers(ops, off)
    host = np.ascontiguousarray(ops)
    wins = windows(n, cuts)
    for k in order:
        lo, hi = wins[k]
        if hi == lo:
            assert f.replay(None, 0, 0, lo, None) == 0
            continue
        p = (host.ctypes.data + lo * OP_BYTES) if feeds == "host" else (src.data_ptr() + off + lo * OP_BYTES)
        q = p if inplace else dst.data_ptr() + off + lo * OP_BYTES
        rc = f.replay(p, hi - lo, 0 if feeds == "host" else 1, lo, q)
        if rc:
            return rc, None
    got = (src if inplace else dst).cpu().numpy()
    assert got[:off].tobytes() == b"\xA5" * off and got[off + n * OP_BYTES:].tobytes() == b"\xA5" * PAD
    return 0, got[off:off + n * OP_BYTES].tobytes()


def test_log_and_replay(rv):
    """after a counting pass the log holds n_rewritten records; replaying windows cut differently from the feeds -- forwards,
    backwards, shuffled, from host and device memory, in place -- gives rv_ops_fold's bytes; replay_end refuses a short round and an
    altered record; without the flag replay is RV_E_ARG"""
    rng = np.random.default_rng(77)
    for name in ("length_513", "known_chain_3000", f"known_layer_{SOLO + 1}", "b2a_64_known", "sizehint_grows", "nothing_known", "one_const", "empty"):
        case = CASES[name]
        _, ops, wc = case
        n = len(ops)
        want, winfo = whole(rv, case)
        rc, out, info, f = run_feeds(rv, ops, wc, sorted(int(x) for x in rng.integers(0, n + 1, 3)), mode="count", flags=1)
        try:
            assert rc == 0 and out == b"\xA5" * len(out)
            rc, fi = f.info()
            assert fi["log_records"] == winfo["n_rewritten"] == info["n_rewritten"]
            assert fi["log_bytes"] % 28 == 0 and (fi["log_bytes"] >= 28 * fi["log_records"]) and (fi["log_bytes"] == 0) == (fi["log_records"] == 0)
            assert fi["log_bytes"] <= 28 * max(1024, 2 * fi["log_records"])
            cuts = sorted(int(x) for x in rng.integers(0, n + 1, 5))
            k = len(cuts) + 1
            for order, kw in ((range(k), {}), (reversed(range(k)), {"feeds": "host", "off": 8}), (rng.permutation(k).tolist(), {"inplace": True})):
                rc, got = replay_all(rv, f, ops, list(order), cuts, **kw)
                assert rc == 0 and got == want, (name, cuts)
                assert f.replay_end() == 0
            if n > 1:
                # a short round, a round that says one window twice, an altered record: refused, and the next round is a new one
                assert replay_all(rv, f, ops, [0], [n // 2])[0] == 0 and f.replay_end() == ARG
                assert replay_all(rv, f, ops, [0, 0, 1], [n // 2])[0] == 0 and f.replay_end() == ARG
                other = ops.copy()
                other["dst"][n - 1] ^= 1
                assert replay_all(rv, f, other, [1, 0], [n // 2])[0] == 0 and f.replay_end() == ARG
                assert replay_all(rv, f, ops, [1, 0], [n // 2])[0] == 0 and f.replay_end() == 0
                host = np.ascontiguousarray(ops)
                assert f.replay(host.ctypes.data, 2, 0, n - 1, None) == ARG  # no output
                _, _, dst = buffers(ops, 0)
                assert f.replay(host.ctypes.data, 2, 0, n - 1, dst.data_ptr()) == ARG  # beyond the list
                assert f.replay_end() == ARG and f.replay_end() == (ARG if n else 0)
        finally:
            f.close()
    case = CASES["length_513"]
    rc, _, _, f = run_feeds(rv, case[1], case[2], [100])
    try:
        assert rc == 0 and f.info()[1]["log_bytes"] == 0
        assert replay_all(rv, f, case[1], [0], [])[0] == ARG and f.replay_end() == ARG
    finally:
        f.close()


def test_fallback(rv, monkeypatch):
    """RV_FOLD_MAX_ROUNDS=3, known_chain_65 in three feeds: the feeds that reach the bound come back from the host sweep with the
    same bytes and log entries, host_feeds counts them, on_device is 0, and the feed that stays below the bound is counted on the
    device"""
    case = CASES["known_chain_65"]
    name, ops, wc = case
    want, winfo = whole(rv, case)
    monkeypatch.setenv("RV_FOLD_MAX_ROUNDS", "3")
    for kw in ({}, {"mode": "inplace"}, {"mode": "count"}, {"feeds": "host", "off": 8}):
        before = launches()
        rc, out, info, f = run_feeds(rv, ops, wc, [3, 40], flags=1, **kw)
        try:
            assert rc == 0 and out == (b"\xA5" * len(out) if kw.get("mode") == "count" else want)
            # (the first feed: Input, Const, one op -- two layers; the others: chains deeper than the bound)
            assert info == dict(winfo, device_rounds=2 + 3 + 3, on_device=0)
            fi = f.info()[1]
            assert fi["host_feeds"] == 2 and fi["feeds"] == 3 and fi["log_records"] == winfo["n_rewritten"]
            after = launches()
            assert after[3] - before[3] == 2 and after[0] - before[0] + after[1] - before[1] == 1
            rc, got = replay_all(rv, f, ops, [1, 0], [33])
            assert rc == 0 and got == want and f.replay_end() == 0
        finally:
            f.close()
    monkeypatch.delenv("RV_FOLD_MAX_ROUNDS")
    info = check(rv, case, [3, 40])
    assert info["device_rounds"] == 2 + 37 + 26


@pytest.mark.parametrize("case", ERRORS, ids=[c[0] for c in ERRORS])
def test_errors(rv, case):
    """the bad op lies in the third feed: its code there, nothing written for that feed, only destroy afterwards"""
    name, ops, wc = case
    n = len(ops)
    want = fold_ref.check(ops, wc)
    bad = next(i for i in range(n) if fold_ref.check(ops[:i + 1], wc))
    cuts = [bad // 2, bad]  # (the third feed begins at the bad op)
    for mode in ("new", "count", "inplace"):
        rc, out, _, f = run_feeds(rv, ops, wc, cuts, mode=mode)
        try:
            assert rc == want != 0, name
            good = rv.fold_ops(ops[:bad], wc)[0].tobytes()
            rest = np.ascontiguousarray(ops[bad:]).tobytes()
            assert out == (good + (rest if mode == "inplace" else b"\xA5" * len(rest)) if mode != "count" else b"\xA5" * len(out)), (name, mode)
            host = np.ascontiguousarray(ops)
            assert f.feed(host.ctypes.data, 1, 0, None) == ARG and f.end()[0] == ARG and f.rewind() == ARG and f.info()[0] == ARG
        finally:
            f.close()


def test_pointers_and_order(rv):
    """a misaligned pointer, host memory passed as device memory, a partial overlap: RV_E_ARG before any launch, and the folder goes
    on; calls out of order are RV_E_ARG and leave the folder as it was"""
    import torch

    case = CASES["length_257"]
    name, ops, wc = case
    n = len(ops)
    want, winfo = whole(rv, case)
    raw, src, dst = buffers(ops, 8)
    p, q = src.data_ptr() + 8, dst.data_ptr() + 8
    host = np.ascontiguousarray(ops)
    f = Folder(rv, wc, 1)
    g = Folder(rv, wc, 2)  # an unknown flag
    assert f.rc == 0 and g.rc == ARG
    try:
        before = launches()
        assert f.feed(p + 4, n, 1, q) == ARG and f.feed(p, n, 1, q + 4) == ARG        # misaligned
        assert f.feed(host.ctypes.data, n, 1, q) == ARG and f.feed(p, n, 1, host.ctypes.data) == ARG  # foreign
        assert f.feed(p, n, 1, p + OP_BYTES) == ARG and f.feed(p + OP_BYTES, n - 1, 1, p) == ARG      # overlapping
        assert f.feed(None, n, 1, q) == ARG and f.feed(p, (1 << 31) - 1, 1, q) == ARG                          # past the allocation
        assert f.feed(host.ctypes.data, n, 0, host.ctypes.data) == ARG                                  # d_out is device memory
        torch.cuda.synchronize()
        assert launches() == before and dst.cpu().numpy().tobytes() == b"\xA5" * len(dst)
        # and the folder goes on
        assert f.feed(p, n, 1, q) == 0 and f.end()[0] == 0 and dst.cpu().numpy()[8:8 + n * OP_BYTES].tobytes() == want
    finally:
        f.close()
    raw, src, dst = buffers(ops, 8)
    p, q = src.data_ptr() + 8, dst.data_ptr() + 8
    f = Folder(rv, wc, 1)
    try:
        # out of order: before the end
        assert f.rewind() == ARG and f.replay(p, 1, 1, 0, q) == ARG and f.replay_end() == ARG
        assert f.feed(p, 100, 1, q) == 0 and f.rewind() == ARG
        assert f.feed(None, 0, 0, None) == 0 and f.feed(p + 100 * OP_BYTES, n - 100, 1, q + 100 * OP_BYTES) == 0
        rc, info = f.end()
        assert rc == 0 and dst.cpu().numpy()[8:8 + n * OP_BYTES].tobytes() == want and {k: info[k] for k in ("n_ops", "n_rewritten", "n_known")} == \
            {k: winfo[k] for k in ("n_ops", "n_rewritten", "n_known")}
        # after the end
        assert f.feed(p, 1, 1, q) == ARG and f.end()[0] == ARG
        assert f.info()[1]["total_ops"] == n
        assert f.replay(p, n, 1, 0, p + OP_BYTES) == ARG and f.replay(p + 4, n, 1, 0, q) == ARG
        assert f.replay(p, n, 1, 0, p) == 0 and f.replay_end() == 0  # in place
        assert src.cpu().numpy()[8:8 + n * OP_BYTES].tobytes() == want
    finally:
        f.close()
    assert rv.Context.default() is not None and Folder(rv, (1 << 31, 0)).rc == 8


# ---- what it is for ----
def test_python_face(rv):
    import torch

    from reverie_amd import fold, prune

    case = CASES["length_513"]
    name, ops, wc = case
    want, winfo = whole(rv, case)
    t = torch.from_numpy(np.ascontiguousarray(ops).view(np.uint8).reshape(-1, OP_BYTES).copy()).cuda()
    with fold.DeviceFolder(wc, keep_log=True) as df:
        outs = [df.feed(ops[:100]), df.feed(t[100:300]), df.feed(t[300:400].clone(), inplace=True)]
        assert df.feed(ops[400:], count_only=True) is None
        info = df.end()
        assert b"".join(o.cpu().numpy().tobytes() for o in outs) == want[:400 * OP_BYTES]
        assert {k: v for k, v in info.items() if k != "device_rounds"} == dict({k: v for k, v in winfo.items() if k != "device_rounds"}, on_device=1)
        assert df.replay(ops[500:], 500).cpu().numpy().tobytes() == want[500 * OP_BYTES:] and df.replay(t[:500], 0).cpu().numpy().tobytes() == want[:500 * OP_BYTES]
        df.replay_end()
        assert df.get_info()["log_records"] == winfo["n_rewritten"]
        df.rewind()
        assert df.feed(t).cpu().numpy().tobytes() == want
        df.end()
    for source in (prune.window_pieces(ops, 200), prune.window_pieces(t, 257)):
        pieces2, finfo = fold.fold_pieces(source, wc)
        try:
            assert {k: finfo[k] for k in winfo if k != "device_rounds"} == dict({k: v for k, v in winfo.items() if k != "device_rounds"}, on_device=1)
            assert finfo["folder"]["log_records"] == winfo["n_rewritten"] and finfo["folder"]["total_ops"] == 513
            for _ in range(2):
                assert b"".join(o.cpu().numpy().tobytes() for o, _ in pieces2()) == want
                back = [o.cpu().numpy().tobytes() for o, _ in pieces2.backwards()]
                assert b"".join(reversed(back)) == want
            n_g = int(np.count_nonzero((ops["domain"] == 0) & (ops["opcode"] == 0)))
            n_z = int(np.count_nonzero((ops["domain"] == 1) & (ops["opcode"] == 0)))
            assert tuple(map(sum, zip(*(c for _, c in pieces2())))) == (n_g, n_z)
            # composes with no further code
            pruned, pinfo = prune.prune_pieces(pieces2, wc)
            try:
                assert b"".join(o.cpu().numpy().tobytes() for o, _ in pruned()) == rv.prune_ops(np.frombuffer(want, OP_DTYPE), wc)[0].tobytes()
            finally:
                pruned.pruner.close()
        finally:
            pieces2.folder.close()


@pytest.mark.parametrize("case", PROOFS, ids=[c[0] for c in PROOFS])
def test_proofs_over_folded_pieces(rv, oracle, rule_seeds, case):
    """prove_streaming_pieces over fold_pieces(window_pieces(ops, w)) is byte for byte the oracle's proof of rv_ops_fold(ops) for the
    same seeds, at two window sizes; it verifies strictly over folded pieces and is not a proof of the original; with prune and
    compact_wires on top it is what the whole-list stream gives with fold, prune and compact_wires; evaluation keeps every
    assertion's result"""
    from reverie_amd import fold, prune, stream

    name, ops, wc, wit_g, wit_z, counts = case
    folded, info = rv.fold_ops(ops, wc)
    want = oracle.prove(folded, wit_g, wit_z, wc, rule_seeds, threads=2)
    want2, winfo2 = rv.prove_streaming(ops, wit_g, wit_z, wc, seeds=rule_seeds, max_chunk_ops=CHUNK, fold=True, prune=True, compact_wires=True)
    for w in (7, 64):
        source = prune.window_pieces(ops, w)
        pieces2, finfo = fold.fold_pieces(source, wc)
        try:
            assert finfo["n_rewritten"] == info["n_rewritten"] > 0
            proof, _ = stream.prove_streaming_pieces(pieces2, wit_g, wit_z, wc, seeds=rule_seeds, max_chunk_ops=CHUNK)
            assert bytes(proof) == want, (name, w)
            assert stream.verify_streaming_pieces(pieces2, wc, want, strict=True, max_chunk_ops=CHUNK)[0]
            try:
                crossed = stream.verify_streaming_pieces(source, wc, want, strict=True, max_chunk_ops=CHUNK)[0]
            except rv.ReverieError:
                crossed = False
            assert not crossed
            both, sinfo = stream.prove_streaming_pieces(pieces2, wit_g, wit_z, wc, seeds=rule_seeds, max_chunk_ops=CHUNK, prune=True, compact_wires=True)
            assert bytes(both) == bytes(want2) and sinfo["prune"]["n_kept"] == winfo2["prune"]["n_kept"], (name, w)
            assert stream.verify_streaming_pieces(pieces2, wc, bytes(want2), max_chunk_ops=CHUNK, prune=True, compact_wires=True)[0]
            ev = stream.evaluate_streaming_pieces(pieces2, wit_g, wit_z, wc, max_chunk_ops=CHUNK)
            plain = stream.evaluate_streaming_pieces(source, wit_g, wit_z, wc, max_chunk_ops=CHUNK)
            assert ev.n_failed.tolist() == plain.n_failed.tolist() == [0]
            bad_g, bad_z = ([1 - wit_g[0]] + list(wit_g[1:]), wit_z) if len(wit_g) else (wit_g, [wit_z[0] + 1] + list(wit_z[1:]))
            ev = stream.evaluate_streaming_pieces(pieces2, bad_g, bad_z, wc, max_chunk_ops=CHUNK)
            plain = stream.evaluate_streaming_pieces(source, bad_g, bad_z, wc, max_chunk_ops=CHUNK)
            assert ev.n_failed.tolist() == plain.n_failed.tolist() and ev.first_failed_op.tolist() == plain.first_failed_op.tolist()
        finally:
            pieces2.folder.close()


def test_command_line(rv, rule_seeds, tmp_path, capfd, monkeypatch):
    """prove and verify with --fold-windows --prune-windows --compact-windows agree with --fold --prune --compact-wires on an rvops
    file; convert writes rv_ops_fold's records"""
    import functools

    from reverie_amd import stream
    from reverie_amd.__main__ import main

    monkeypatch.setattr(stream, "prove_streaming_pieces", functools.partial(stream.prove_streaming_pieces, seeds=rule_seeds))
    name, ops, wc, wit_g, _, _ = PROOFS[0]
    prog, wit = str(tmp_path / "p.rvops"), str(tmp_path / "w.txt")
    ops.tofile(prog)
    open(wit, "w").write("".join(str(b) for b in wit_g))
    proofs, lines = {}, {}
    for tag, flags in (("whole", ["--fold", "--prune", "--compact-wires"]), ("windows", ["--fold-windows", "--prune-windows", "--compact-windows"])):
        out = str(tmp_path / (tag + ".proof"))
        base = ["--program-path", prog, "--program-format", "rvops", "--stream"]
        assert main(["--operation", "prove", "--witness-path", wit, "--proof-path", out] + base + flags) == 0
        err = capfd.readouterr().err
        lines[tag] = [ln for ln in err.split("\n") if ln.startswith(("fold:", "prune:", "compact-wires:"))]
        assert err.index("fold:") < err.index("prune:") < err.index("compact-wires:")
        assert main(["--operation", "verify", "--proof-path", out] + base + flags) == 0
        assert [ln for ln in capfd.readouterr().err.split("\n") if ln.startswith(("fold:", "prune:", "compact-wires:"))] == lines[tag]
        proofs[tag] = open(out, "rb").read()
    assert proofs["whole"] == proofs["windows"] and lines["whole"] == lines["windows"]
    conv = ["--operation", "convert", "--program-path", prog, "--program-format", "rvops", "--output-format", "rvops"]
    assert main(conv + ["--output-path", str(tmp_path / "a.rvops"), "--fold"]) == 0
    assert main(conv + ["--output-path", str(tmp_path / "b.rvops"), "--fold-windows"]) == 0
    a, b = open(str(tmp_path / "a.rvops"), "rb").read(), open(str(tmp_path / "b.rvops"), "rb").read()
    assert a == b == rv.fold_ops(ops, wc)[0].tobytes()
    assert main(["--operation", "oneshot", "--evaluator", "stream", "--witness-path", wit, "--program-path", prog, "--program-format", "rvops",
                 "--fold-windows", "--prune-windows"]) == 0
