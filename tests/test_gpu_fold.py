"""rv_ops_fold_device (the kernels of csrc/fold_dev.hip) against rv_ops_fold, the host definition that tests/test_fold_host.py pins to
the Python model: records and info byte for byte on the cases of tests/fold_cases.py and the generated lists, with d_out 16-byte
aligned and 8 bytes off, the layer counts against the model's, in place, the counting call, the launches, the pointer rules, the
fall-back; then what folding is for: the proof of the folded list, the streams and the linker's blocks."""
import ctypes as C
import os

import numpy as np
import pytest

import fold_cases as fc
import fold_ref
from reverie_amd.ops import OP_DTYPE

pytestmark = pytest.mark.gpu

OP_BYTES = OP_DTYPE.itemsize
PAD = 88  # bytes behind the list in the output tensors (at least 64, and no multiple of the record size)
CHUNK = 1024


def _solo_limit():
    from reverie_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    lim = (C.c_uint32 * 5)()
    assert _lib.lib().rv_hook_fold_limits(lim) == 0
    return int(lim[1])


SOLO = _solo_limit()
CORPUS = fc.corpus(SOLO)
ERRORS = fc.error_cases()
PROOFS = fc.proof_programs()
_layers = {}


@pytest.fixture(scope="module")
def rv():
    import reverie_amd

    reverie_amd.Context.default()
    return reverie_amd


def on_device(prog):
    import torch

    return torch.from_numpy(np.ascontiguousarray(prog).view(np.uint8).reshape(-1, OP_BYTES).copy()).cuda()


def layers(case):
    """the model's layer widths of a case, computed once"""
    if case[0] not in _layers:
        _layers[case[0]] = fold_ref.layers(case[1])[1]
    return _layers[case[0]]


def launches():
    from reverie_amd import _lib

    out = (C.c_uint64 * 4)()
    assert _lib.lib().rv_hook_fold_launches(out) == 0
    return [int(x) for x in out]


def run_device(rv, ops, wc, mode="new", off=0):
    """one rv_ops_fold_device call on a copy of ops in GPU memory -> (rc, record bytes, bytes behind the list, info).  mode "new": the
    output tensor is filled with 0xA5 and longer than the list, and d_out begins `off` bytes (a multiple of 8) into it; "inplace":
    d_out is d_ops, which lies `off` bytes into its tensor; "count": d_out is NULL."""
    import torch

    from reverie_amd import _lib

    n = len(ops)
    raw = np.ascontiguousarray(ops).view(np.uint8).reshape(-1)
    src = torch.full((off + n * OP_BYTES + PAD,), 0xA5, dtype=torch.uint8, device="cuda")
    src[off:off + n * OP_BYTES] = torch.from_numpy(raw.copy()).cuda()
    dst = torch.full((off + n * OP_BYTES + PAD,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    fi = _lib.FoldInfo()
    d_ops = C.c_void_p(src.data_ptr() + off) if n else None
    d_out = None if mode == "count" or not n else d_ops if mode == "inplace" else C.c_void_p(dst.data_ptr() + off)
    rc = _lib.lib().rv_ops_fold_device(rv.Context.default().handle, d_ops, n, int(wc[0]), int(wc[1]), d_out, C.byref(fi))
    got_src, got = src.cpu().numpy(), dst.cpu().numpy()
    assert got_src[:off].tobytes() == b"\xA5" * off and got_src[off + n * OP_BYTES:].tobytes() == b"\xA5" * PAD
    if mode != "inplace":
        assert got_src[off:off + n * OP_BYTES].tobytes() == raw.tobytes()  # the input is read only
    else:
        got = got_src
    assert got[:off].tobytes() == b"\xA5" * off
    info = {k: int(getattr(fi, k)) for k, _ in fi._fields_}
    return rc, got[off:off + n * OP_BYTES].tobytes(), got[off + n * OP_BYTES:].tobytes(), info


def check(rv, case, off=0, mode="new"):
    name, ops, wc = case
    want, winfo = rv.fold_ops(ops, wc)
    widths = layers(case)
    before = launches()
    rc, out, tail, info = run_device(rv, ops, wc, mode, off)
    after = launches()
    assert rc == 0, (name, rc)
    if mode == "count":
        assert out == b"\xA5" * len(out), name
    else:
        assert out == want.tobytes(), name
    assert tail == b"\xA5" * PAD, name  # nothing behind the list
    assert info == dict(winfo, device_rounds=len(widths), on_device=1), (name, info, winfo, len(widths))
    assert after[3] == before[3], name
    if not widths:
        assert after[2] == before[2], name  # a list with nothing known costs no propagation launch
    else:
        assert after[2] > before[2], name
    # (a list with nothing known and no read of an unwritten index is copied: neither a rewrite nor a counting launch)
    assert (after[0] - before[0], after[1] - before[1]) in ((0, 0), (0, 1) if mode == "count" else (1, 0)), name
    if winfo["n_rewritten"] or winfo["n_known"]:
        assert after[0] - before[0] + after[1] - before[1] == 1, name
    return want, winfo


@pytest.mark.parametrize("case", CORPUS, ids=[c[0] for c in CORPUS])
def test_device_equals_host(rv, case):
    check(rv, case)


def test_output_eight_bytes_off(rv):
    """d_out on an address that is 8 modulo 16: every tile's image lies at the other shift"""
    for case in CORPUS:
        check(rv, case, off=8)


@pytest.mark.parametrize("off", [0, 8])
def test_generated_lists(rv, off):
    """the issue's generator, 400 lists: device == host, layer counts == the model's"""
    for case in fc.generated():
        check(rv, case, off=off)


def test_in_place(rv):
    """d_out == d_ops, on both alignments: a tile writes the records it read"""
    for case in CORPUS:
        if len(case[1]):
            check(rv, case, off=8 * (len(case[1]) & 1), mode="inplace")


def test_counting_call(rv):
    """d_out NULL: the same numbers, no rewrite launch, nothing written"""
    for case in CORPUS:
        if len(case[1]):
            check(rv, case, mode="count")


def test_launches_by_frontier(rv):
    """a list with nothing known makes no propagation launch; a layer of at most the solo limit and a layer one wider are both
    propagated on the device (the hook counts solo and wide launches together: the layer count tells that each was stepped), and the
    host looks again only after a whole interval of launches"""
    from reverie_amd import _lib

    cases = {c[0]: c for c in CORPUS}
    lim = (C.c_uint32 * 5)()
    assert _lib.lib().rv_hook_fold_limits(lim) == 0
    before = launches()
    check(rv, cases["nothing_known"])
    assert launches() == before  # (copied: no rewrite launch either)
    for name in (f"known_layer_{SOLO}", f"known_layer_{SOLO + 1}"):
        before = launches()
        _, info = check(rv, cases[name])
        after = launches()
        assert info["n_known"] == int(name.rsplit("_", 1)[1]) + 1
        assert after[2] - before[2] == 2 * lim[2] and after[3] == before[3], name  # one interval: a solo and a wide launch per iteration
    before = launches()
    check(rv, cases["widen_past_solo_and_narrow"])
    assert launches()[2] - before[2] >= 2 * lim[2]


def test_device_rounds(rv):
    """device_rounds is the model's layer count on the chain and layer cases (check() compares them on every case)"""
    cases = {c[0]: c for c in CORPUS}
    for depth in (1, 2, 63, 64, 65, 3000):
        assert check(rv, cases[f"known_chain_{depth}"])[1]["n_known"] == depth and len(layers(cases[f"known_chain_{depth}"])) == depth
    for w in (SOLO - 1, SOLO, SOLO + 1):
        assert layers(cases[f"known_layer_{w}"]) == [1, w]
        check(rv, cases[f"known_layer_{w}"])
    assert len(layers(cases["widen_past_solo_and_narrow"])) == 23


@pytest.mark.parametrize("case", ERRORS, ids=[c[0] for c in ERRORS])
def test_errors(rv, case):
    """the host call's code, d_out untouched"""
    name, ops, wc = case
    want = fold_ref.check(ops, wc)
    with pytest.raises(rv.ReverieError) as e:
        rv.fold_ops(ops, wc)
    assert e.value.code == want != 0
    for mode in ("new", "count", "inplace"):
        rc, out, tail, _ = run_device(rv, ops, wc, mode)
        assert rc == want and tail == b"\xA5" * PAD, name
        assert out == (np.ascontiguousarray(ops).tobytes() if mode == "inplace" else b"\xA5" * len(out)), name


def test_pointer_checks(rv):
    """a partial overlap of d_out and d_ops, a misaligned pointer, host memory, a range past the allocation: RV_E_ARG before a launch"""
    import torch

    from reverie_amd import _lib

    ops, wc = fc.known_chain(50)
    n = len(ops)
    f = _lib.lib().rv_ops_fold_device
    h = rv.Context.default().handle
    src = torch.full((2 * n * OP_BYTES + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    src[8:8 + n * OP_BYTES] = torch.from_numpy(ops.view(np.uint8).reshape(-1).copy()).cuda()
    dst = torch.full((n * OP_BYTES + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    p, q = src.data_ptr() + 8, dst.data_ptr()
    before = launches()

    def call(d_ops=p, d_out=q, ctx=h, n_ops=n):
        return f(ctx, C.c_void_p(d_ops) if d_ops else None, n_ops, wc[0], wc[1], C.c_void_p(d_out) if d_out else None, None)

    assert call(d_out=p + OP_BYTES) == 9                    # a partial overlap
    assert call(d_out=p + (n - 1) * OP_BYTES) == 9          # the last record
    assert call(d_out=p - 8) == 9                           # room that reaches into the list from the front
    assert call(d_ops=p + 4) == 9 and call(d_out=q + 4) == 9  # misaligned
    assert call(d_ops=None) == 9 and call(ctx=None) == 9
    hostmem = ops.copy()
    assert call(d_ops=hostmem.ctypes.data) == 9 and call(d_out=hostmem.ctypes.data) == 9
    assert call(n_ops=(1 << 31) - 1) == 9 and call(n_ops=1 << 31) == 8  # past the allocation; more than the call takes
    if torch.cuda.device_count() > 1:
        other = torch.full((n * OP_BYTES,), 0xA5, dtype=torch.uint8, device="cuda:1")
        torch.cuda.synchronize(1)
        assert call(d_ops=other.data_ptr()) == 9 and call(d_out=other.data_ptr()) == 9
    torch.cuda.synchronize()
    assert launches() == before
    assert dst.cpu().numpy().tobytes() == b"\xA5" * (n * OP_BYTES + 64) and hostmem.tobytes() == ops.tobytes()
    assert src.cpu().numpy()[8:8 + n * OP_BYTES].tobytes() == ops.tobytes()
    want = rv.fold_ops(ops, wc)[0].tobytes()
    assert call(d_out=p + n * OP_BYTES) == 0  # right behind the list is no overlap
    assert src.cpu().numpy()[8 + n * OP_BYTES:8 + 2 * n * OP_BYTES].tobytes() == want
    assert call(d_out=p) == 0  # in place
    assert src.cpu().numpy()[8:8 + n * OP_BYTES].tobytes() == want


def test_fallback_bound(rv, monkeypatch):
    """RV_FOLD_MAX_ROUNDS=3: the depth-65 chain comes back from the host sweep with the same bytes and on_device == 0; at the
    default it is propagated on the device, 65 layers"""
    case = {c[0]: c for c in CORPUS}["known_chain_65"]
    name, ops, wc = case
    want, winfo = rv.fold_ops(ops, wc)
    monkeypatch.setenv("RV_FOLD_MAX_ROUNDS", "3")
    before = launches()
    for mode in ("new", "count", "inplace"):
        rc, out, tail, info = run_device(rv, ops, wc, mode)
        assert rc == 0 and info == dict(winfo, device_rounds=3, on_device=0) and tail == b"\xA5" * PAD
        assert out == (b"\xA5" * len(out) if mode == "count" else want.tobytes())
    assert launches()[3] == before[3] + 3 and launches()[0] == before[0] and launches()[1] == before[1]
    # exactly as many layers as the bound allows stay on the device
    three = fc.known_chain(3)
    rc, out, _, info = run_device(rv, three[0], three[1])
    assert rc == 0 and info["on_device"] == 1 and info["device_rounds"] == 3 and out == rv.fold_ops(three[0], three[1])[0].tobytes()
    monkeypatch.delenv("RV_FOLD_MAX_ROUNDS")
    rc, out, _, info = run_device(rv, ops, wc)
    assert rc == 0 and info == dict(winfo, device_rounds=65, on_device=1) and out == want.tobytes()


def test_python_front_end(rv):
    import torch

    case = {c[0]: c for c in CORPUS}["length_513"]
    name, ops, wc = case
    want, winfo = rv.fold_ops(ops, wc)
    assert winfo["n_rewritten"] > 0
    for t in (on_device(ops), on_device(ops).reshape(-1), on_device(ops).view(torch.int64)):
        out, info = rv.fold_ops(t, wc)
        assert out.device == t.device and out.dtype == torch.uint8 and tuple(out.shape) == (len(want), OP_BYTES) and out.is_contiguous()
        assert out.cpu().numpy().tobytes() == want.tobytes() and out.data_ptr() != t.data_ptr()
        assert info == dict(winfo, device_rounds=info["device_rounds"], on_device=1)
        assert t.cpu().numpy().tobytes() == ops.tobytes()
        none, info2 = rv.fold_ops(t, wc, count_only=True)
        assert none is None and info2 == info
        same, info3 = rv.fold_ops(t, wc, inplace=True)
        assert same is t and info3 == info and t.cpu().numpy().tobytes() == want.tobytes()
    with pytest.raises(ValueError):
        rv.fold_ops(on_device(ops))
    with pytest.raises(rv.ReverieError) as e:
        rv.fold_ops(on_device(ops), (1, 1))
    assert e.value.code == fold_ref.WIRE_OOB


@pytest.mark.parametrize("case", PROOFS, ids=[c[0] for c in PROOFS])
def test_proof_parity(rv, oracle, rule_seeds, case):
    """Proof.new on the device-folded list is byte for byte the oracle's proof of the host-folded list with the same seeds, verifies
    strictly, is shorter than the proof of the original and is not a proof of the original; the streams fold first"""
    name, ops, wc, wit_g, wit_z, counts = case
    folded, info = rv.fold_ops(ops, wc)
    d_folded, d_info = rv.fold_ops(on_device(ops), wc)
    assert d_folded.cpu().numpy().tobytes() == folded.tobytes() and info["n_rewritten"] > 0
    want = oracle.prove(folded, wit_g, wit_z, wc, rule_seeds, threads=2)
    circuit = rv.Circuit.from_device_ops(d_folded, wc, device_z64=True, device_b2a=True)
    proof = rv.Proof.new(circuit, wit_g, wit_z, seeds=rule_seeds)
    assert bytes(proof) == want
    assert proof.verify(circuit, strict=True) and proof.verify(rv.Circuit(folded, wc), strict=True)
    original = rv.Circuit(ops, wc)
    assert len(want) < len(bytes(rv.Proof.new(original, wit_g, wit_z, seeds=rule_seeds)))
    try:
        crossed = proof.verify(original, strict=True)
    except rv.ReverieError:
        crossed = False
    assert not crossed
    # the streams: fold=True runs first, then the pruning, then the compaction; prover and verifier both fold
    pruned = rv.prune_ops(folded, wc)[0]
    want2 = oracle.prove(pruned, wit_g, wit_z, wc, rule_seeds, threads=2)
    for src in (ops, on_device(ops)):
        got, sinfo = rv.prove_streaming(src, wit_g, wit_z, wc, seeds=rule_seeds, max_chunk_ops=CHUNK, fold=True)
        assert bytes(got) == want and "prune" not in sinfo, name
        assert {k: v for k, v in sinfo["fold"].items() if k not in ("device_rounds", "on_device")} == {k: v for k, v in info.items() if
                                                                                                     k not in ("device_rounds", "on_device")}
        assert rv.verify_streaming(src, wc, want, max_chunk_ops=CHUNK, fold=True)[0]
        got, sinfo = rv.prove_streaming(src, wit_g, wit_z, wc, seeds=rule_seeds, max_chunk_ops=CHUNK, fold=True, prune=True, compact_wires=True)
        assert bytes(got) == want2 and len(want2) < len(want) and sinfo["prune"]["n_kept"] == len(pruned) and "compact" in sinfo, name
        assert rv.verify_streaming(src, wc, want2, max_chunk_ops=CHUNK, fold=True, prune=True, compact_wires=True)[0]
        plain, pinfo = rv.prove_streaming(src, wit_g, wit_z, wc, seeds=rule_seeds, max_chunk_ops=CHUNK)
        assert "fold" not in pinfo and len(bytes(plain)) > len(want)


def test_block_folded_on_device(rv):
    """Block.folded() on a device block: the host block's folded records, left in GPU memory, with the same ports"""
    from reverie_amd.ops import GF2, program

    ops = program([GF2.Input(0), GF2.Input(1), GF2.Const(2, 1), GF2.Const(3, 0), GF2.Mul(4, 0, 2), GF2.Mul(5, 1, 3), GF2.Mul(6, 0, 1), GF2.Add(7, 4, 5),
                   GF2.Add(8, 7, 6), GF2.Sub(9, 2, 8)])
    want = rv.Block(ops, (0, 10), outputs=[8, 9]).folded()
    got = rv.Block(on_device(ops), (0, 10), n_ports=2, outputs=[8, 9]).folded()
    assert got.on_device and got.ops.cpu().numpy().tobytes() == want.ops.tobytes() and len(got) == len(want) == len(ops)
    assert (got.n_ports, got.wire_counts, got.outputs) == (want.n_ports, want.wire_counts, want.outputs)
    assert got.fold_info["on_device"] == 1 and got.fold_info["n_rewritten"] == want.fold_info["n_rewritten"] == 4
