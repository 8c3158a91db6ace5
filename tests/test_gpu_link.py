"""rv_link_plan_* against rv_link (the host definition, itself pinned to the numpy model of tests/link_ref.py by
tests/test_link_host.py): the whole list and its info on every case of tests/link_cases.py -- tables and blocks from the host and from
GPU memory, d_ops aligned and 8 bytes off, guard bytes around the range -- every range of a case of about 40 records and the ranges
around every tile edge, ordinals beyond 2^32, the error rule, and the adder chain from a plan to a proof, whole and streamed."""
import ctypes as C

import numpy as np
import pytest

import link_cases as lc
import link_ref
from reverie_amd import _lib
from reverie_amd.ops import OP_DTYPE

pytestmark = pytest.mark.gpu
REC = OP_DTYPE.itemsize
GUARD = 4  # records of guard on each side of a range


@pytest.fixture(scope="module")
def ctx():
    import reverie_amd

    return reverie_amd.Context.default()


@pytest.fixture(scope="module")
def T():
    out = (C.c_uint32 * 2)()
    assert _lib.lib().rv_hook_link_tiles(out) == 0
    return int(out[0])


@pytest.fixture(scope="module")
def cases(T):
    """[(name, Spec, the host's list, the host's info)], computed once"""
    out = []
    for name, spec in lc.ok_cases(T):
        ops, info = lc.to_netlist(spec).link_host()
        out.append((name, spec, ops, info))
    return out


def emit_guarded(plan, first, n, offset):
    """records [first, first + n) into the middle of a pre-filled buffer, `offset` (0 or 8) bytes off a 16-byte boundary
    -> (the range's bytes, its Input counts); the bytes around the range must be untouched"""
    import torch

    buf = torch.full(((n + 2 * GUARD) * REC + 16,), 0xA5, dtype=torch.uint8, device=f"cuda:{plan.ctx.device}")
    start = (-buf.data_ptr()) % 16 + offset + GUARD * REC
    assert (buf.data_ptr() + start) % 16 == offset % 16
    plan.emit(first, n, buf[start:start + n * REC])
    host = buf.cpu().numpy()
    assert (host[:start] == 0xA5).all() and (host[start + n * REC:] == 0xA5).all(), (first, n, offset)
    return host[start:start + n * REC].tobytes(), plan.last_piece


def counts_of(ops):
    inp = link_ref.is_input(ops)
    return int(np.count_nonzero(inp & (ops["domain"] == 0))), int(np.count_nonzero(inp & (ops["domain"] == 1)))


@pytest.mark.parametrize("tables,blocks", [("host", "host"), ("device", "host"), ("host", "device"), ("device", "device")])
def test_whole_list_is_the_host_s(ctx, cases, tables, blocks):
    dev = f"cuda:{ctx.device}"
    for name, spec, want, winfo in cases:
        nl = lc.to_netlist(spec, dev if tables == "device" else None, dev if blocks == "device" else None)
        with nl.plan(ctx) as plan:
            assert plan.info == winfo, (name, plan.info, winfo)
            for offset in (0, 8):
                got, counts = emit_guarded(plan, 0, winfo["n_ops"], offset)
                assert got == want.tobytes(), (name, offset)
                assert counts == (winfo["n_input_gf2"], winfo["n_input_z64"]), name
            assert plan.link_device().cpu().numpy().tobytes() == want.tobytes(), name


def test_every_range_of_forty(ctx, cases):
    name, spec, want, winfo = [c for c in cases if c[0] == "forty"][0]
    n_ops = winfo["n_ops"]
    assert 36 <= n_ops <= 48
    with lc.to_netlist(spec).plan(ctx) as plan:
        for first in range(n_ops + 1):
            for n in range(n_ops - first + 1):
                got, counts = emit_guarded(plan, first, n, 8 * ((first + n) & 1))
                model, mcounts = link_ref.link_range(spec, first, n)
                assert got == model.tobytes() == want[first:first + n].tobytes(), (first, n)
                assert counts == mcounts == counts_of(want[first:first + n]), (first, n)


def test_ranges_around_tile_edges(ctx, cases, T):
    name, spec, want, winfo = [c for c in cases if c[0] == f"total-{2 * T + 1}"][0]
    n_ops = winfo["n_ops"]
    edges = [0, 1, T - 1, T, T + 1, 2 * T - 1, 2 * T, n_ops - 1, n_ops]
    with lc.to_netlist(spec).plan(ctx) as plan:
        for first in edges:
            for end in edges:
                for n in {end - first, end - first + 1, T, T + 1, 1} if end >= first else ():
                    if n < 0 or first + n > n_ops:
                        continue
                    got, counts = emit_guarded(plan, first, n, 8 * (first & 1))
                    model, mcounts = link_ref.link_range(spec, first, n)
                    assert got == model.tobytes() == want[first:first + n].tobytes(), (first, n)
                    assert counts == mcounts, (first, n)


def test_ordinals_beyond_2_32(ctx):
    """a fabricated non-SSA block of 2^20 records over 16 wires, instanced 4 100 times: 1 000 records on each side of ordinal 2^32
    against the model's range (which never makes the whole list)"""
    import torch

    rng = np.random.default_rng(11)
    n, inst = 1 << 20, 4100
    blk = np.zeros(n, OP_DTYPE)
    blk["opcode"] = rng.choice([2, 6, 3], n)
    for f in ("dst", "a", "b"):
        blk[f] = rng.integers(0, 16, n)
    blk["imm"] = rng.integers(0, 2, n)
    ports = np.arange(0, n, 4096)
    blk["opcode"][ports] = 0
    blk["a"][ports] = blk["b"][ports] = blk["imm"][ports] = 0
    k = np.arange(len(ports) * inst, dtype=np.uint32)
    bindings = np.where(k % 3 == 0, np.uint32(link_ref.WITNESS), k % 16).astype(np.uint32)
    spec = link_ref.Spec([(blk, (0, 16))], np.zeros(inst, np.uint32), bindings, head=[lc.GF2.Input(0)], gf2_base=1)
    dev = f"cuda:{ctx.device}"
    nl = lc.to_netlist(spec, dev, dev)
    with nl.plan(ctx) as plan:
        assert plan.info["n_ops"] == 1 + n * inst > 1 << 32 and plan.info["gf2_wires"] == 1 + 16 * inst
        assert plan.info["n_input_gf2"] == 1 + int(np.count_nonzero(bindings == link_ref.WITNESS))
        for first, count in (((1 << 32) - 1000, 2000), ((1 << 32) - 1, 2), (1 << 32, 1), (plan.info["n_ops"] - 300, 300)):
            model, mcounts = link_ref.link_range(spec, first, count)
            got, counts = emit_guarded(plan, first, count, 8)
            assert got == model.tobytes() and counts == mcounts, first
    torch.cuda.empty_cache()


@pytest.mark.parametrize("name,spec,code", lc.bad_cases(), ids=[c[0] for c in lc.bad_cases()])
def test_codes_are_the_host_s(ctx, name, spec, code):
    from reverie_amd import ReverieError

    dev = f"cuda:{ctx.device}"
    for tables, blocks in ((None, None), (dev, dev)):
        with pytest.raises(ReverieError) as host:
            lc.to_netlist(spec).link_host()
        with pytest.raises(ReverieError) as e:
            lc.to_netlist(spec, tables, blocks).plan(ctx)
        assert e.value.code == host.value.code == code
    # no plan is made: the handle stays NULL
    d, flags, _, _keep = lc.to_netlist(spec)._desc(ctx, False)
    handle = C.c_void_p(1)
    assert _lib.lib().rv_link_plan_create(ctx.handle, C.byref(d), C.c_uint32(flags), C.byref(handle)) == code and not handle


def test_refused_calls_touch_nothing(ctx, cases):
    import torch

    L = _lib.lib()
    name, spec, want, winfo = [c for c in cases if c[0] == "forty"][0]
    n_ops = winfo["n_ops"]
    nl = lc.to_netlist(spec)
    d, flags, _, _keep = nl._desc(ctx, False)
    handle = C.c_void_p()
    assert L.rv_link_plan_create(ctx.handle, C.byref(d), C.c_uint32(4), C.byref(handle)) == link_ref.ARG and not handle  # an unknown flag
    assert L.rv_link_plan_create(ctx.handle, C.byref(d), C.c_uint32(_lib.RV_LINK_BLOCKS_ON_DEVICE), C.byref(handle)) == link_ref.ARG  # host blocks
    assert L.rv_link_plan_create(ctx.handle, C.byref(d), C.c_uint32(_lib.RV_LINK_TABLES_ON_DEVICE), C.byref(handle)) == link_ref.ARG and not handle
    assert L.rv_link_plan_create(None, C.byref(d), C.c_uint32(0), C.byref(handle)) == link_ref.ARG
    assert L.rv_link_plan_create(ctx.handle, None, C.c_uint32(0), C.byref(handle)) == link_ref.ARG
    with nl.plan(ctx) as plan:
        buf = torch.full(((n_ops + 1) * REC,), 0x5A, dtype=torch.uint8, device=f"cuda:{ctx.device}")
        host = np.zeros(n_ops * REC, np.uint8)
        piece = _lib.LinkPiece()
        p = buf.data_ptr()
        for first, n, ptr in ((n_ops + 1, 0, p), (0, n_ops + 1, p), (n_ops, 1, p), (1 << 63, 1 << 63, p), (0, 4, p + 4), (0, 4, p + 12), (0, 4, None),
                              (0, n_ops, host.ctypes.data)):
            rc = L.rv_link_plan_emit(plan.handle, C.c_uint64(first), C.c_uint64(n), C.c_void_p(ptr), C.byref(piece))
            assert rc == link_ref.ARG, (first, n)
        assert L.rv_link_plan_emit(plan.handle, C.c_uint64(0), C.c_uint64(1), C.c_void_p(p), None) == link_ref.ARG
        assert L.rv_link_plan_emit(None, C.c_uint64(0), C.c_uint64(1), C.c_void_p(p), C.byref(piece)) == link_ref.ARG
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == 0x5A).all() and not host.any()
        # a range of no record at all is a call like any other
        assert L.rv_link_plan_emit(plan.handle, C.c_uint64(n_ops), C.c_uint64(0), None, C.byref(piece)) == 0
        assert (piece.first_op, piece.n_ops, piece.n_input_gf2, piece.n_input_z64) == (n_ops, 0, 0, 0)
    # one call stays below 2^28 records: decided before the buffer is looked at
    spec = link_ref.Spec([lc.EMPTY_WIDE, ([lc.GF2.Const(0, 1)] * 4096, (0, 1))], [1] * (1 << 16), [])
    with lc.to_netlist(spec).plan(ctx) as plan:
        assert plan.info["n_ops"] == 1 << 28
        rc = L.rv_link_plan_emit(plan.handle, C.c_uint64(0), C.c_uint64(1 << 28), C.c_void_p(buf.data_ptr()), C.byref(piece))
        assert rc == link_ref.UNSUPPORTED
    assert (buf.cpu().numpy() == 0x5A).all()


def test_adder_chain_from_plan_to_proof(ctx, rule_seeds):
    """the linked list proves and verifies where it lies; whole, in pieces of 100 records and compacted in windows it gives the bytes
    of Proof.new on the host-linked list; a witness with one flipped bit fails one AssertZero, at its op index"""
    import reverie_amd as rv
    from reverie_amd import stream

    nl_host, _, tail, bits, total = lc.adder_chain()
    nl_host.set_tail(tail(total))
    ops, info = nl_host.link_host()
    wc = info["wire_counts"]
    wit = np.asarray(bits, np.uint8)
    want = bytes(rv.Proof.new(rv.Circuit(ops, wc, ctx), wit, [], seeds=rule_seeds))
    nl, _, tail_d, _, _ = lc.adder_chain(device=True)  # (the block parsed on the GPU: its records never reach the host)
    nl.set_tail(tail_d(total))
    with nl.plan(ctx) as plan:
        assert plan.info == info
        linked = plan.link_device()
        assert linked.cpu().numpy().tobytes() == ops.tobytes()
        circuit = rv.Circuit.from_device_ops(linked, wc, ctx)
        proof = rv.Proof.new(circuit, wit, [], seeds=rule_seeds)
        assert bytes(proof) == want and proof.verify(circuit, strict=True)
        pieces = plan.pieces(100)
        assert sum(len(t) for t, _ in pieces()) == info["n_ops"]
        assert tuple(map(sum, zip(*(c for _, c in pieces())))) == (info["n_input_gf2"], info["n_input_z64"])
        streamed, _ = stream.prove_streaming_pieces(pieces, wit, [], wc, seeds=rule_seeds, ctx=ctx)
        assert bytes(streamed) == want
        ok, _ = stream.verify_streaming_pieces(pieces, wc, streamed, ctx=ctx)
        assert ok
        compacted, cinfo = stream.prove_streaming_pieces(pieces, wit, [], wc, seeds=rule_seeds, ctx=ctx, compact_wires=True)
        assert bytes(compacted) == want and cinfo["compact"]["gf2_wires"] < wc[1]
        assert stream.evaluate_streaming_pieces(pieces, wit, [], wc, ctx=ctx).n_failed.tolist() == [0]
        bad = wit.copy()
        bad[64 * 3 + 63] ^= 1  # the top bit of a word: the sum moves by 2^63, so exactly the last output bit differs
        ev = stream.evaluate_streaming_pieces(pieces, bad, [], wc, ctx=ctx)
        assert ev.n_failed.tolist() == [1] and ev.first_failed_op.tolist() == [info["n_ops"] - 1]
