"""rv_ops_compact_wires_device (the kernels of csrc/compact_dev.hip) against the rule as plain Python (tests/compact_ref.py), byte for
byte, on the corpus of the host test and at the lengths and shapes where the parallel form can go wrong; then what the compaction
is for: the same proofs, the same evaluation, a smaller wire store."""
import ctypes as C

import numpy as np
import pytest

import circuits
import compact_cases
import compact_ref
from reverie_amd.ops import GF2, OP_DTYPE, program

pytestmark = pytest.mark.gpu

OP_BYTES = OP_DTYPE.itemsize
T = compact_cases.TILE
CHUNK = 1024
PAD = 88  # bytes behind the list in the output tensor (at least 64, and no multiple of the record size)
CORPUS = compact_cases.corpus()
ERRORS = compact_cases.error_cases()
INFO_FIELDS = ("z64_wires", "gf2_wires", "gf2_pinned", "gf2_zero_wire", "z64_zero_wire", "gf2_values", "z64_values")


@pytest.fixture(scope="module")
def rv():
    import reverie_amd

    reverie_amd.Context.default()
    return reverie_amd


def on_device(prog):
    """the packed records of a numpy program as a torch tensor in GPU memory ([n, 24] uint8)"""
    import torch

    return torch.from_numpy(np.ascontiguousarray(prog).view(np.uint8).reshape(-1, OP_BYTES).copy()).cuda()


def run_device(rv, prog, wc, in_place=False):
    """-> (rc, the n records written, the bytes behind them, info) of one rv_ops_compact_wires_device call on a copy of prog in GPU
    memory; the output tensor is filled with 0xA5 and PAD bytes longer than the list (in_place: d_out = d_ops)"""
    import torch

    from reverie_amd import _lib

    n = len(prog)
    src = torch.full((n * OP_BYTES + PAD,), 0xA5, dtype=torch.uint8, device="cuda")
    src[:n * OP_BYTES] = torch.from_numpy(np.ascontiguousarray(prog).view(np.uint8).reshape(-1).copy()).cuda()
    dst = src if in_place else torch.full((n * OP_BYTES + PAD,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ci = _lib.CompactInfo()
    rc = _lib.lib().rv_ops_compact_wires_device(rv.Context.default().handle, C.c_void_p(src.data_ptr()), n, int(wc[0]), int(wc[1]),
                                                C.c_void_p(dst.data_ptr()), C.byref(ci))
    if not in_place:
        assert src.cpu().numpy()[:n * OP_BYTES].tobytes() == np.ascontiguousarray(prog).tobytes()  # the input is read only
    got = dst.cpu().numpy()
    return rc, got[:n * OP_BYTES].tobytes(), got[n * OP_BYTES:].tobytes(), {k: int(getattr(ci, k)) for k in INFO_FIELDS}


def check(rv, prog, wc):
    rc_ref, want, counts, info = compact_ref.compact(prog, wc)
    assert rc_ref == 0
    for in_place in (False, True):
        rc, out, tail, got = run_device(rv, prog, wc, in_place)
        assert rc == 0
        assert out == want.tobytes()
        assert tail == b"\xA5" * PAD
        assert got == info
    return counts


@pytest.mark.parametrize("name,prog,wc", CORPUS, ids=[c[0] for c in CORPUS])
def test_device_equals_reference(rv, name, prog, wc):
    check(rv, prog, wc)


@pytest.mark.parametrize("n", [0, 1, 2, T - 1, T, T + 1, 3 * T + 5])
def test_lengths_around_a_workgroup(rv, n):
    prog, wc = compact_cases.of_length(n, seed=n)
    assert len(prog) == n
    check(rv, prog, wc)


def test_70000_ops(rv):
    """several workgroups of every scan, op indices past 2^16; both domains, heavy reuse"""
    prog, wc = compact_cases.of_length(70_000, seed=7)
    check(rv, prog, wc)


def test_reuse_chain_of_5000(rv):
    """every value takes its predecessor's slot one op late: a parent chain 5 000 long, 13 doubling rounds"""
    prog, wc = compact_cases.chain(5000)
    assert check(rv, prog, wc) == (0, 2)


@pytest.mark.parametrize("name,prog,wc,code", ERRORS, ids=[c[0] for c in ERRORS])
def test_errors(rv, name, prog, wc, code):
    """the compiler's code (the host sweep's, which tests/test_compact_wires_host.py pins to the oracle's), d_out untouched"""
    from reverie_amd import _lib

    want = compact_ref.compact(prog, wc)[0]
    assert want in (3, 5) and (code is None or code == want)
    host = np.empty_like(prog)
    assert _lib.lib().rv_ops_compact_wires(prog.ctypes.data_as(C.c_void_p), len(prog), wc[0], wc[1], host.ctypes.data_as(C.c_void_p), None) == want
    handle = C.c_void_p()
    assert _lib.lib().rv_circuit_compile(rv.Context.default().handle, prog.ctypes.data_as(C.c_void_p), C.c_size_t(len(prog)), C.c_size_t(wc[0]),
                                         C.c_size_t(wc[1]), C.byref(handle)) == want
    rc, out, tail, _ = run_device(rv, prog, wc)
    assert rc == want
    assert out == b"\xA5" * len(out) and tail == b"\xA5" * PAD
    rc, out, tail, _ = run_device(rv, prog, wc, in_place=True)
    assert rc == want and out == prog.tobytes() and tail == b"\xA5" * PAD


def test_first_error_wins_across_workgroups(rv):
    """two bad ops many workgroups apart, the later one met first by the hardware or not: the earlier op's code"""
    good, wc = compact_cases.of_length(5 * T, seed=5)
    for first, second, want in (((0, 77, 0, 1, 0, 0, 0), GF2.Add(24, 0, 1), 5), (GF2.Add(24, 0, 1), (0, 77, 0, 1, 0, 0, 0), 3)):
        prog = good.copy()
        prog[T + 3] = np.array([first], OP_DTYPE)[0]
        prog[4 * T + 9] = np.array([second], OP_DTYPE)[0]
        rc, out, _, _ = run_device(rv, prog, wc)
        assert rc == want and out == b"\xA5" * len(out)


def test_pointer_checks(rv):
    """a misaligned pointer, host memory, another device's memory, a range past the allocation: RV_E_ARG, nothing written"""
    import torch

    from reverie_amd import _lib

    prog, wc = compact_cases.chain(50)
    n = len(prog)
    f = _lib.lib().rv_ops_compact_wires_device
    h = rv.Context.default().handle
    ci = _lib.CompactInfo()
    src = torch.full((n * OP_BYTES + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    src[4:4 + n * OP_BYTES] = torch.from_numpy(prog.view(np.uint8).reshape(-1).copy()).cuda()
    dst = torch.full((n * OP_BYTES + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    p, q = src.data_ptr(), dst.data_ptr()
    assert f(h, C.c_void_p(p + 4), n, wc[0], wc[1], C.c_void_p(q), C.byref(ci)) == 9
    assert f(h, C.c_void_p(p + 8), n, wc[0], wc[1], C.c_void_p(q + 4), C.byref(ci)) == 9
    assert f(h, None, n, wc[0], wc[1], C.c_void_p(q), C.byref(ci)) == 9
    assert f(h, C.c_void_p(p + 8), n, wc[0], wc[1], None, C.byref(ci)) == 9
    assert f(None, C.c_void_p(p + 8), n, wc[0], wc[1], C.c_void_p(q), C.byref(ci)) == 9
    host = prog.copy()
    assert f(h, host.ctypes.data_as(C.c_void_p), n, wc[0], wc[1], C.c_void_p(q), C.byref(ci)) == 9
    assert f(h, C.c_void_p(p + 8), n, wc[0], wc[1], host.ctypes.data_as(C.c_void_p), C.byref(ci)) == 9
    # a list that would end some 48 GiB behind the tensors' allocations (the longest the call takes: 2^31 ops are RV_E_UNSUPPORTED)
    far = (1 << 31) - 1
    assert f(h, C.c_void_p(p + 8), far, wc[0], wc[1], C.c_void_p(q), C.byref(ci)) == 9
    assert f(h, C.c_void_p(p + 8), far + 1, wc[0], wc[1], C.c_void_p(q), C.byref(ci)) == 8
    # a partial overlap of input and output
    assert f(h, C.c_void_p(p + 8), 2, 0, 8, C.c_void_p(p + 8 + OP_BYTES), C.byref(ci)) == 9
    if torch.cuda.device_count() > 1:
        other = torch.full((n * OP_BYTES,), 0xA5, dtype=torch.uint8, device="cuda:1")
        torch.cuda.synchronize(1)
        assert f(h, C.c_void_p(other.data_ptr()), n, wc[0], wc[1], C.c_void_p(q), C.byref(ci)) == 9
        assert f(h, C.c_void_p(p + 8), n, wc[0], wc[1], C.c_void_p(other.data_ptr()), C.byref(ci)) == 9
        assert other.cpu().numpy().tobytes() == b"\xA5" * (n * OP_BYTES)
    torch.cuda.synchronize()
    assert dst.cpu().numpy().tobytes() == b"\xA5" * (n * OP_BYTES + 64)
    assert host.tobytes() == prog.tobytes()


def test_python_front_end(rv):
    import torch

    prog, _, wc, _ = circuits.layered_gf2(n_in=64, width=256, layers=12, fold_to=16)
    want = compact_ref.compact(prog, wc)[1]
    for t in (on_device(prog), on_device(prog).reshape(-1), on_device(prog).view(torch.int64)):
        out, counts, info = rv.compact_wires(t, wc)
        assert counts == (0, 298) and info["gf2_values"] == 3392
        assert out.shape == t.shape and out.dtype == t.dtype and out.device == t.device and out.data_ptr() != t.data_ptr()
        assert out.cpu().numpy().tobytes() == want.tobytes()
        assert t.cpu().numpy().tobytes() == prog.tobytes()
    with pytest.raises(ValueError):
        rv.compact_wires(on_device(prog))
    with pytest.raises(rv.ReverieError) as e:
        rv.compact_wires(on_device(prog), (0, 100))
    assert e.value.code == 3


def parity_programs():
    p, w, c, _ = circuits.layered_gf2(n_in=64, width=256, layers=12, fold_to=16)
    out = [("layered_gf2_ssa", p, w, [], c)]
    for s in range(2):
        p, w2, w64, c = circuits.random_mixed(np.random.default_rng(80 + s), n_gates=150)
        out.append((f"random_mixed_{s}", p, w2, w64, c))
    return out


PARITY = parity_programs()


@pytest.mark.parametrize("device_compile", [False, True])
@pytest.mark.parametrize("name,prog,w2,w64,wc", PARITY, ids=[c[0] for c in PARITY])
def test_proof_parity(rv, rule_seeds, name, prog, w2, w64, wc, device_compile):
    flags = dict(device_compile=True, device_z64=True, device_b2a=True) if device_compile else {}
    want = bytes(rv.Proof.new(rv.Circuit(prog, wc, **flags), w2, w64, seeds=rule_seeds))
    new, counts, _ = rv.compact_wires(prog, wc)
    d_new, d_counts, _ = rv.compact_wires(on_device(prog), wc)
    assert d_counts == counts and d_new.cpu().numpy().tobytes() == new.tobytes()
    assert bytes(rv.Proof.new(rv.Circuit(new, counts, **flags), w2, w64, seeds=rule_seeds)) == want
    assert bytes(rv.Proof.new(rv.Circuit.from_device_ops(d_new, counts, device_z64=True, device_b2a=True), w2, w64, seeds=rule_seeds)) == want
    full = rv.largest_wires(prog)  # (a stream takes no SizeHint that grows a count: the uncompacted list begins with the grown counts)
    for ops in (prog, on_device(prog)):
        plain, info0 = rv.prove_streaming(ops, w2, w64, full, seeds=rule_seeds, max_chunk_ops=CHUNK, **flags)
        small, info1 = rv.prove_streaming(ops, w2, w64, wc, seeds=rule_seeds, max_chunk_ops=CHUNK, compact_wires=True, **flags)
        assert bytes(plain) == want and bytes(small) == want
        assert "compact" not in info0 and (info1["compact"]["z64_wires"], info1["compact"]["gf2_wires"]) == counts
        assert rv.verify_streaming(ops, wc, want, max_chunk_ops=CHUNK, compact_wires=True, **flags)[0]
        assert not rv.verify_streaming(ops, wc, want[:-1] + bytes([want[-1] ^ 1]), max_chunk_ops=CHUNK, compact_wires=True, **flags)[0]
    # the original proof against the compacted program, and the batch forms
    assert rv.Proof(want).verify(rv.Circuit(new, counts), strict=True)
    g = np.tile(np.asarray(w2, np.uint8), (2, 1))
    z = np.tile(np.asarray(w64, np.uint64), (2, 1))
    binfo = {}
    pair = rv.prove_streaming_batch(prog, g, z, wc, seeds=np.stack([rule_seeds, rule_seeds[::-1]]), max_chunk_ops=CHUNK, info=binfo, compact_wires=True)
    assert bytes(pair[0]) == want and (binfo["compact"]["z64_wires"], binfo["compact"]["gf2_wires"]) == counts
    assert rv.verify_streaming_batch(prog, wc, pair, max_chunk_ops=CHUNK, compact_wires=True) == [True, True]


def last_writers(prog, domain):
    """op index -> dst for the ops that are the last to write their destination in `domain` (0: GF(2); 1: Z64, B2A included)"""
    last = {}
    for i, (dom, opc, dst) in enumerate(zip(prog["domain"].tolist(), prog["opcode"].tolist(), prog["dst"].tolist())):
        if (dom == domain and opc != 8) or (dom == 2 and domain == 1):
            last[dst] = i
    return {i: w for w, i in last.items()}


@pytest.mark.parametrize("name,prog,w2,w64,wc", PARITY, ids=[c[0] for c in PARITY])
def test_evaluation_parity(rv, name, prog, w2, w64, wc):
    if np.isin(1, prog["opcode"][prog["domain"] <= 1]):  # (no clear evaluation of Random ops: they become constants here)
        prog = prog.copy()
        prog["opcode"][(prog["domain"] <= 1) & (prog["opcode"] == 1)] = 9
    new, counts, _ = rv.compact_wires(prog, wc)
    for ops in (prog, on_device(prog)):
        old = rv.evaluate_streaming(ops, w2, w64, rv.largest_wires(prog), max_chunk_ops=CHUNK, values=True)
        info = {}
        got = rv.evaluate_streaming(ops, w2, w64, wc, max_chunk_ops=CHUNK, values=True, info=info, compact_wires=True)
        assert (info["compact"]["z64_wires"], info["compact"]["gf2_wires"]) == counts
        assert got.gf2.shape == (1, counts[1]) and got.z64.shape == (1, counts[0])
        assert got.ok.tolist() == old.ok.tolist() and got.n_failed.tolist() == old.n_failed.tolist()
        assert got.first_failed_op.tolist() == old.first_failed_op.tolist()
        # an op that is the last writer of its destination under both numberings: the same value at the old and the new dst
        for domain, a, b in ((0, old.gf2, got.gf2), (1, old.z64, got.z64)):
            lo, ln = last_writers(prog, domain), last_writers(new, domain)
            both = sorted(set(lo) & set(ln))
            assert both or not lo
            assert [int(a[0, lo[i]]) for i in both] == [int(b[0, ln[i]]) for i in both]


def test_stream_memory(rv, rule_seeds):
    prog, wit, wc, _ = circuits.layered_gf2(n_in=64, width=256, layers=12)
    ssa, info0 = rv.prove_streaming(prog, wit, [], wc, seeds=rule_seeds, max_chunk_ops=CHUNK)
    small, info1 = rv.prove_streaming(prog, wit, [], wc, seeds=rule_seeds, max_chunk_ops=CHUNK, compact_wires=True)
    assert bytes(small) == bytes(ssa)
    assert info1["compact"]["gf2_wires"] == compact_ref.compact(prog, wc)[2][1]
    assert info1["wire_store_bytes"] < info0["wire_store_bytes"]
    prog16, wit16, wc16, _ = circuits.layered_gf2(n_in=64, width=256, layers=12, fold_to=16)
    assert rv.prove_streaming(on_device(prog16), wit16, [], wc16, seeds=rule_seeds, max_chunk_ops=CHUNK, compact_wires=True)[1]["compact"]["gf2_wires"] == 298
