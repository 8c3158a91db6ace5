"""rv_ops_prune_device (the kernels of csrc/prune_dev.hip) against rv_ops_prune, the host definition that tests/test_prune_host.py pins
to the Python models: records, old_index and info byte for byte on the cases of tests/prune_cases.py and the generated lists, the
layer counts against the peeling model, the counting call, the pointer rules, the fall-back; then what pruning is for: the proof of
the pruned list, the same evaluation, the streams and the linker's blocks."""
import ctypes as C

import numpy as np
import pytest

import prune_cases as pc
import prune_ref
from reverie_amd.ops import OP_DTYPE

pytestmark = pytest.mark.gpu

OP_BYTES = OP_DTYPE.itemsize
PAD = 88  # bytes behind the capacity in the output tensors (at least 64, and no multiple of the record size)
CORPUS = pc.corpus()
ERRORS = pc.error_cases()
PROOFS = pc.proof_programs()
CHUNK = 1024


@pytest.fixture(scope="module")
def rv():
    import reverie_amd

    reverie_amd.Context.default()
    return reverie_amd


def on_device(prog):
    import torch

    return torch.from_numpy(np.ascontiguousarray(prog).view(np.uint8).reshape(-1, OP_BYTES).copy()).cuda()


def host(rv, ops, wc, og=(), oz=()):
    """rv_ops_prune through the package -> (records, info, old_index)"""
    return rv.prune_ops(ops, wc, og, oz)


def launches():
    from reverie_amd import _lib

    out = (C.c_uint64 * 4)()
    assert _lib.lib().rv_hook_prune_launches(out) == 0
    return [int(x) for x in out]


def run_device(rv, ops, wc, og=(), oz=(), cap=None, count_only=False, off=0):
    """one rv_ops_prune_device call on a copy of ops in GPU memory -> (rc, n_out, record bytes, bytes behind the capacity, old_index,
    entries behind the capacity, info).  The output tensors are filled with 0xA5 and longer than the capacity; off: d_out begins that
    many bytes (a multiple of 8) into its tensor."""
    import torch

    from reverie_amd import _lib

    n = len(ops)
    cap = n if cap is None else cap
    src = on_device(ops) if n else torch.zeros((1, OP_BYTES), dtype=torch.uint8, device="cuda")
    dst = torch.full((off + cap * OP_BYTES + PAD,), 0xA5, dtype=torch.uint8, device="cuda")
    old = torch.full((cap + 16,), -1515870811, dtype=torch.int32, device="cuda")  # 0xA5A5A5A5
    g, z = np.asarray(og, np.uint32), np.asarray(oz, np.uint32)
    torch.cuda.synchronize()
    pi, n_out = _lib.PruneInfo(), C.c_size_t(12345)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
    rc = _lib.lib().rv_ops_prune_device(rv.Context.default().handle, C.c_void_p(src.data_ptr()) if n else None, n, int(wc[0]), int(wc[1]), p(g), g.size,
                                        p(z), z.size, None if count_only else C.c_void_p(dst.data_ptr() + off), cap, C.byref(n_out),
                                        None if count_only else C.c_void_p(old.data_ptr()), C.byref(pi))
    if n:
        assert src.cpu().numpy().tobytes() == np.ascontiguousarray(ops).tobytes()  # the input is read only
    got, got_old = dst.cpu().numpy(), old.cpu().numpy().view(np.uint32)
    assert got[:off].tobytes() == b"\xA5" * off
    info = {k: int(getattr(pi, k)) for k, _ in pi._fields_}
    return rc, int(n_out.value), got[off:off + cap * OP_BYTES].tobytes(), got[off + cap * OP_BYTES:].tobytes(), got_old[:cap], got_old[cap:], info


def check(rv, case, off=0):
    name, ops, wc, og, oz = case
    want, winfo, wold = host(rv, ops, wc, og, oz)
    layers = prune_ref.peel(ops, og, oz)[1]["device_rounds"]
    before = launches()
    rc, n_out, out, tail, old, old_tail, info = run_device(rv, ops, wc, og, oz, off=off)
    after = launches()
    assert rc == 0, (name, rc)
    k = len(want)
    assert n_out == k and out[:k * OP_BYTES] == want.tobytes(), name
    assert out[k * OP_BYTES:] == b"\xA5" * (len(out) - k * OP_BYTES) and tail == b"\xA5" * PAD, name  # nothing behind the kept records
    assert (old[:k] == wold).all() and (old[k:] == 0xA5A5A5A5).all() and (old_tail == 0xA5A5A5A5).all(), name
    assert info == dict(winfo, device_rounds=layers, on_device=1), (name, info, winfo, layers)
    assert after[3] == before[3] and after[0] - before[0] == (1 if len(ops) else 0), name
    if layers == 0:
        assert after[2] == before[2], name  # a list with nothing dead costs no round at all
    return want, winfo


@pytest.mark.parametrize("case", CORPUS, ids=[c[0] for c in CORPUS])
def test_device_equals_host(rv, case):
    check(rv, case)


def test_output_eight_bytes_off(rv):
    """d_out on an address that is 8 modulo 16: every tile's image lies at the other shift"""
    cases = {c[0]: c for c in CORPUS}
    for name in ("alignments", "length_2049", "b2a_ranges"):
        check(rv, cases[name], off=8)


def test_generated_lists(rv):
    """the issue's generator, 400 lists: device == host, layer counts == the peeling model's"""
    for case in pc.generated():
        check(rv, case)


def test_counting_call(rv):
    """d_out NULL: the same numbers, no emit launch, nothing written"""
    for case in CORPUS:
        name, ops, wc, og, oz = case
        if not 0 < len(ops) <= 5000:
            continue
        _, winfo, _ = host(rv, ops, wc, og, oz)
        before = launches()
        rc, n_out, out, tail, old, _, info = run_device(rv, ops, wc, og, oz, count_only=True)
        after = launches()
        assert rc == 0 and n_out == winfo["n_kept"], name
        assert {k: v for k, v in info.items() if k not in ("device_rounds", "on_device")} == {k: v for k, v in winfo.items() if k not in ("device_rounds", "on_device")}
        assert info["on_device"] == 1 and info["device_rounds"] == prune_ref.peel(ops, og, oz)[1]["device_rounds"], name
        assert after[0] == before[0] and after[1] == before[1] + 1, name
        assert out == b"\xA5" * len(out) and tail == b"\xA5" * PAD and (old == 0xA5A5A5A5).all(), name


def test_capacity(rv):
    """a capacity below the number kept: RV_E_ARG, nothing written; exactly enough: the records"""
    case = {c[0]: c for c in CORPUS}["length_2049"]
    name, ops, wc, og, oz = case
    want, _, wold = host(rv, ops, wc, og, oz)
    k = len(want)
    rc, n_out, out, tail, old, old_tail, _ = run_device(rv, ops, wc, og, oz, cap=k - 1)
    assert rc == prune_ref.ARG and out == b"\xA5" * len(out) and tail == b"\xA5" * PAD and (old == 0xA5A5A5A5).all()
    rc, n_out, out, tail, old, old_tail, _ = run_device(rv, ops, wc, og, oz, cap=k)
    assert rc == 0 and n_out == k and out == want.tobytes() and tail == b"\xA5" * PAD and (old == wold).all() and (old_tail == 0xA5A5A5A5).all()


@pytest.mark.parametrize("case", ERRORS, ids=[c[0] for c in ERRORS])
def test_errors(rv, case):
    """the host call's code (rv_ops_compact_wires' on the list, then RV_E_ARG for an output out of range), d_out untouched"""
    name, ops, wc, og, oz, _ = case
    want = prune_ref.check(ops, wc, og, oz)
    with pytest.raises(rv.ReverieError) as e:
        host(rv, ops, wc, og, oz)
    assert e.value.code == want != 0
    for count_only in (False, True):
        rc, n_out, out, tail, old, _, _ = run_device(rv, ops, wc, og, oz, count_only=count_only)
        assert rc == want and n_out == 12345 and out == b"\xA5" * len(out) and tail == b"\xA5" * PAD and (old == 0xA5A5A5A5).all(), name


def test_pointer_checks(rv):
    """any overlap of d_out and d_ops, a misaligned pointer, host memory, a range past the allocation: RV_E_ARG before a launch"""
    import torch

    from reverie_amd import _lib

    ops, wc = pc.dead_chain(50)
    n = len(ops)
    f = _lib.lib().rv_ops_prune_device
    h = rv.Context.default().handle
    src = torch.full((2 * n * OP_BYTES + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    src[8:8 + n * OP_BYTES] = torch.from_numpy(ops.view(np.uint8).reshape(-1).copy()).cuda()
    dst = torch.full((n * OP_BYTES + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    old = torch.full((n + 16,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    p, q, o = src.data_ptr() + 8, dst.data_ptr(), old.data_ptr()
    before = launches()

    def call(d_ops=p, d_out=q, d_old=o, cap=n, ctx=h, n_ops=n):
        return f(ctx, C.c_void_p(d_ops) if d_ops else None, n_ops, wc[0], wc[1], None, 0, None, 0, C.c_void_p(d_out) if d_out else None, cap, None,
                 C.c_void_p(d_old) if d_old else None, None)

    assert call(d_out=p) == 9                               # in place
    assert call(d_out=p + OP_BYTES) == 9                    # a partial overlap
    assert call(d_out=p + (n - 1) * OP_BYTES) == 9          # the last record
    assert call(d_out=p - 8, cap=1) == 9                    # one record of room that reaches into the list
    assert call(d_ops=p + 4) == 9 and call(d_out=q + 4) == 9 and call(d_old=o + 2) == 9  # misaligned
    assert call(d_ops=None) == 9 and call(ctx=None) == 9
    hostmem = ops.copy()
    assert call(d_ops=hostmem.ctypes.data) == 9 and call(d_out=hostmem.ctypes.data) == 9
    assert call(d_old=np.zeros(n, np.uint32).ctypes.data) == 9
    assert call(n_ops=(1 << 31) - 1) == 9 and call(n_ops=1 << 31) == 8  # past the allocation; more than the call takes
    assert call(cap=1 << 40) == 9                                        # room the allocation does not have
    assert f(h, C.c_void_p(p), n, wc[0], wc[1], None, 1, None, 0, None, 0, None, None, None) == 9  # a NULL list with a count
    if torch.cuda.device_count() > 1:
        other = torch.full((n * OP_BYTES,), 0xA5, dtype=torch.uint8, device="cuda:1")
        torch.cuda.synchronize(1)
        assert call(d_ops=other.data_ptr()) == 9 and call(d_out=other.data_ptr()) == 9
    torch.cuda.synchronize()
    assert launches() == before
    assert dst.cpu().numpy().tobytes() == b"\xA5" * (n * OP_BYTES + 64) and (old.cpu().numpy() == 7).all() and hostmem.tobytes() == ops.tobytes()
    assert call(d_out=p + n * OP_BYTES) == 0  # right behind the list is no overlap
    assert src.cpu().numpy()[8 + n * OP_BYTES:8 + n * OP_BYTES + 6 * OP_BYTES].tobytes() == rv.prune_ops(ops, wc)[0].tobytes()


def test_fallback_bound(rv, monkeypatch):
    """RV_PRUNE_MAX_ROUNDS=3: the depth-5 000 chain comes back from the host sweep with the same bytes and on_device == 0; at the
    default it is peeled on the device, 5 000 layers"""
    case = {c[0]: c for c in CORPUS}["dead_chain_5000"]
    name, ops, wc, og, oz = case
    want, winfo, wold = host(rv, ops, wc, og, oz)
    monkeypatch.setenv("RV_PRUNE_MAX_ROUNDS", "3")
    before = launches()
    for count_only in (False, True):
        rc, n_out, out, tail, old, _, info = run_device(rv, ops, wc, og, oz, count_only=count_only)
        assert rc == 0 and n_out == len(want) and info == dict(winfo, device_rounds=3, on_device=0)
        if not count_only:
            assert out[:n_out * OP_BYTES] == want.tobytes() and (old[:n_out] == wold).all() and tail == b"\xA5" * PAD
    assert launches()[3] == before[3] + 2 and launches()[0] == before[0]
    # exactly as many layers as the bound allows stay on the device
    three = pc.dead_chain(3)
    rc, n_out, out, _, _, _, info = run_device(rv, three[0], three[1])
    assert rc == 0 and info["on_device"] == 1 and info["device_rounds"] == 3
    monkeypatch.delenv("RV_PRUNE_MAX_ROUNDS")
    rc, n_out, out, _, _, _, info = run_device(rv, ops, wc, og, oz)
    assert rc == 0 and info == dict(winfo, device_rounds=5000, on_device=1) and out[:n_out * OP_BYTES] == want.tobytes()


def test_python_front_end(rv):
    import torch

    case = {c[0]: c for c in CORPUS}["length_2049"]
    name, ops, wc, og, oz = case
    want, winfo, wold = host(rv, ops, wc, og, oz)
    for t in (on_device(ops), on_device(ops).reshape(-1), on_device(ops).view(torch.int64)):
        out, info, old = rv.prune_ops(t, wc, og, oz)
        assert out.device == t.device and out.dtype == torch.uint8 and tuple(out.shape) == (len(want), OP_BYTES) and out.is_contiguous()
        assert out.cpu().numpy().tobytes() == want.tobytes() and (old.cpu().numpy().view(np.uint32) == wold).all()
        assert info["on_device"] == 1 and info["n_kept"] == winfo["n_kept"]
        assert t.cpu().numpy().tobytes() == ops.tobytes()
        none, info2, none2 = rv.prune_ops(t, wc, og, oz, count_only=True)
        assert none is None and none2 is None and info2 == info
    with pytest.raises(ValueError):
        rv.prune_ops(on_device(ops))
    with pytest.raises(rv.ReverieError) as e:
        rv.prune_ops(on_device(ops), wc, [wc[1]])
    assert e.value.code == prune_ref.ARG
    # a result of less than half the list gives the list's room back
    chain, cwc = pc.dead_chain(5000)
    out, info, old = rv.prune_ops(on_device(chain), cwc)
    assert out.shape[0] == 6 and out.untyped_storage().nbytes() < 1024 and old.cpu().numpy().tolist() == [0, 1, 2, 3, 4, 5]


@pytest.mark.parametrize("case", PROOFS, ids=[c[0] for c in PROOFS])
def test_proof_parity(rv, oracle, rule_seeds, case):
    """Proof.new on the device-pruned list is byte for byte the oracle's proof of the host-pruned list with the same seeds, verifies
    strictly, is shorter than the proof of the original and is not a proof of the original"""
    name, ops, wc, wit_g, wit_z = case
    pruned, info, _ = host(rv, ops, wc)
    d_pruned, d_info, _ = rv.prune_ops(on_device(ops), wc)
    assert d_pruned.cpu().numpy().tobytes() == pruned.tobytes() and info["n_dropped"] > 0
    want = oracle.prove(pruned, wit_g, wit_z, wc, rule_seeds, threads=2)
    circuit = rv.Circuit.from_device_ops(d_pruned, wc, device_z64=True, device_b2a=True)
    proof = rv.Proof.new(circuit, wit_g, wit_z, seeds=rule_seeds)
    assert bytes(proof) == want
    assert proof.verify(circuit, strict=True) and proof.verify(rv.Circuit(pruned, wc), strict=True)
    original = rv.Circuit(ops, wc)
    assert len(want) < len(bytes(rv.Proof.new(original, wit_g, wit_z, seeds=rule_seeds)))
    try:
        crossed = proof.verify(original, strict=True)
    except rv.ReverieError:
        crossed = False
    assert not crossed
    # the streams: prune=True runs first, then the compaction; prover and verifier both prune
    full = rv.largest_wires(ops)
    for src in (ops, on_device(ops)):
        got, sinfo = rv.prove_streaming(src, wit_g, wit_z, full, seeds=rule_seeds, max_chunk_ops=CHUNK, prune=True, compact_wires=True)
        assert bytes(got) == want, name
        assert sinfo["prune"]["n_kept"] == len(pruned) and sinfo["prune"]["n_dropped"] == info["n_dropped"] and "compact" in sinfo
        assert rv.verify_streaming(src, full, want, max_chunk_ops=CHUNK, prune=True, compact_wires=True)[0]
        plain, pinfo = rv.prove_streaming(src, wit_g, wit_z, full, seeds=rule_seeds, max_chunk_ops=CHUNK)
        assert "prune" not in pinfo and len(bytes(plain)) > len(want)


def test_evaluate_batch_agrees(rv):
    """Circuit.evaluate_batch on the original and on the device-pruned list: the same failing counts for 8 witnesses, some failing;
    the first failing op maps back through old_index"""
    name, ops, wc, wit_g, wit_z = PROOFS[0]
    ops = ops.copy()
    ops["opcode"][(ops["domain"] <= 1) & (ops["opcode"] == 1)] = 9  # (no clear evaluation of a Random: a constant here; it is dead)
    d_pruned, info, d_old = rv.prune_ops(on_device(ops), wc)
    old = d_old.cpu().numpy().view(np.uint32)
    wits = np.tile(np.asarray(wit_g, np.uint8), (8, 1))
    wits[1::3, 0] ^= 1
    a = rv.Circuit(ops, wc).evaluate_batch(wits)
    b = rv.Circuit.from_device_ops(d_pruned, wc).evaluate_batch(wits)
    assert a.n_failed.tolist() == b.n_failed.tolist() and 0 < int(np.count_nonzero(a.n_failed)) < 8
    for fa, fb in zip(a.first_failed_op.tolist(), b.first_failed_op.tolist()):
        assert (fa == -1) == (fb == -1) and (fb == -1 or int(old[fb]) == fa)


def test_block_pruned_on_device(rv):
    """Block.pruned() on a device block: the host block's pruned records, left in GPU memory, with the same ports"""
    import bristol_gen

    text = bristol_gen.adder64()
    host_block = rv.Block.from_bristol(text)
    dev_block = rv.Block.from_bristol(text, device=True)
    half = host_block.outputs[:32]
    want = rv.Block(host_block.ops, host_block.wire_counts, outputs=half).pruned()
    got = rv.Block(dev_block.ops, dev_block.wire_counts, n_ports=dev_block.n_ports, outputs=half).pruned()
    assert got.on_device and got.ops.cpu().numpy().tobytes() == want.ops.tobytes() and len(got) == len(want) < len(host_block)
    assert (got.n_ports, got.wire_counts, got.outputs) == (want.n_ports, want.wire_counts, want.outputs)
    assert got.prune_info["on_device"] == 1 and got.prune_info["n_dropped"] == want.prune_info["n_dropped"] > 0
