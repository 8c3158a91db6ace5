"""The linker's cases (tests/test_link_host.py, tests/test_gpu_link.py, tests/link_model.cpp): small netlists around the emit
kernel's tile, and one netlist per error code and per order between two errors.  TEST INFRASTRUCTURE."""
from __future__ import annotations

import struct

import numpy as np

import bristol_gen
from link_ref import ARG, BAD, OOB, UNSUPPORTED, WITNESS, Spec, check, is_input, prog
from reverie_amd.ops import B2A, GF2, Z64, SizeHint

GARBAGE = 0xDEADBEEF


def _garbage(op, **fields):
    """an op tuple with fields that name no wire overwritten"""
    names = ("domain", "opcode", "reserved", "dst", "a", "b", "imm")
    rec = list(op)
    for k, v in fields.items():
        rec[names.index(k)] = v
    return tuple(rec)


# ---- the blocks ----
EMPTY = ([], (0, 0))
EMPTY_WIDE = ([], (2, 3))  # no record, but a share of the numbering
ONE = ([GF2.Input(0)], (0, 1))
THREE = ([GF2.Input(0), GF2.Input(1), GF2.Add(2, 0, 1)], (0, 3))
ZTHREE = ([Z64.Input(0), Z64.Input(1), Z64.Mul(2, 0, 1)], (3, 0))
NONSSA = ([GF2.Input(0), GF2.Input(1), GF2.Add(0, 0, 1), GF2.Mul(1, 0, 1), GF2.Add(0, 0, 1), GF2.AssertZero(1)], (0, 2))


def every_opcode(garbage: bool):
    """every opcode of both domains and a B2A; garbage: the fields that name no wire hold some"""
    g = (lambda op, **f: _garbage(op, **f)) if garbage else (lambda op, **f: op)
    ops = []
    for D in (GF2, Z64):
        ops += [g(D.Input(0), a=GARBAGE, b=7, imm=GARBAGE << 8), g(D.Random(1), a=5, b=GARBAGE, imm=3), D.Add(2, 0, 1),
                g(D.AddConst(3, 2, 1), b=GARBAGE), D.Sub(4, 3, 2), g(D.SubConst(5, 4, 1), b=9), D.Mul(6, 5, 4), g(D.MulConst(7, 6, 1), b=GARBAGE),
                g(D.AssertZero(7), dst=GARBAGE, b=11, imm=GARBAGE), g(D.Const(8, 1), a=GARBAGE, b=GARBAGE), g(D.Input(9), a=1, b=2, imm=3)]
    ops.append(g(B2A(10, 6), opcode=77, b=GARBAGE, imm=GARBAGE))
    return (ops, (11, 70))


def bind(blocks, block_of, mode, head=(), tail=(), z64_base=0, gf2_base=0):
    """a Spec whose ports are bound by `mode`: "none", "all" (to wires spread over the result's counts) or "alt" (every other one)"""
    s = Spec(blocks, block_of, [], head, tail, z64_base, gf2_base)
    doms = [o["domain"][is_input(o)] for o, _ in s.blocks]
    dom = np.concatenate([doms[b] for b in block_of] + [np.zeros(0, np.uint8)])
    s.bindings = np.full(len(dom), WITNESS, dtype=np.uint32)
    code, info = check(s)
    assert code == 0, code
    if mode != "none" and len(dom):
        k = np.arange(len(dom), dtype=np.uint64)
        count = np.where(dom == 0, info["gf2_wires"], info["z64_wires"]).astype(np.uint64)
        val = ((k * np.uint64(2654435761)) % np.maximum(count, 1)).astype(np.uint32)
        take = np.ones(len(dom), bool) if mode == "all" else (k % 2 == 1)
        s.bindings = np.where(take & (count > 0), val, s.bindings).astype(np.uint32)
    return s


def _filler(n, base=0):
    """n head or tail records in global numbering"""
    return [GF2.Const(base + (i % 3), i & 1) if i % 4 else GF2.Input(base + (i % 3)) for i in range(n)]


def ok_cases(T: int):
    """[(name, Spec)]; T: the emit kernel's tile"""
    cases = [
        ("nothing", Spec()),
        ("no-instances-blocks-only", Spec([THREE, EMPTY])),
        ("head-and-tail-only", Spec([THREE], [], [], _filler(5), [GF2.AssertZero(2), SizeHint(4, 9), Z64.Input(3)])),
        ("head-only", Spec([], [], [], _filler(3))),
        ("one-instance", bind([THREE], [0], "none")),
        ("one-instance-bound", bind([THREE], [0], "all", head=_filler(4), gf2_base=3)),
        ("one-empty-instance", bind([EMPTY_WIDE], [0], "none")),
    ]
    # blocks of 0, 1 and 3 records instanced 600 times: many instances per tile, empty ones at the start, in the middle, at the end
    of = [0] * 10 + [1] * 140 + [0] * 300 + [2] * 140 + [0] * 10
    assert len(of) == 600
    cases.append(("600-instances-of-0-1-3", bind([EMPTY_WIDE, ONE, THREE], of, "alt")))
    cases.append(("600-one-record-instances", bind([ONE], [0] * 600, "alt", head=_filler(2))))
    cases.append(("600-empty-instances", bind([EMPTY, EMPTY_WIDE], [0, 1] * 300, "none", head=_filler(2), tail=_filler(2))))
    # totals around one and two tiles
    for total in (T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1):
        m = (total - 4) // 3
        cases.append((f"total-{total}", bind([THREE], [0] * m, "alt", head=_filler(2), tail=_filler(total - 2 - 3 * m, 1))))
    # instance boundaries at a tile's first and last record
    cases.append(("instance-ends-with-the-tile", bind([THREE], [0] * 4, "all", head=_filler(T - 3), gf2_base=3)))
    cases.append(("instance-begins-at-the-tile-end", bind([THREE], [0] * 4, "all", head=_filler(T - 1), gf2_base=3)))
    cases.append(("instances-fill-tiles", bind([(THREE[0] + [GF2.Mul(2, 2, 0)], (0, 3))], [0] * (T // 2), "alt")))
    cases.append(("head-and-tail-end-in-one-tile", bind([THREE], [0], "alt", head=_filler(5), tail=_filler(4), gf2_base=3)))
    cases.append(("tile-of-head-instances-tail", bind([ONE, EMPTY], [0, 1, 0, 1, 1, 0], "none", head=_filler(T - 4, 1), tail=_filler(T, 2), gf2_base=8)))
    # block types interleaved
    cases.append(("two-types", bind([THREE, ZTHREE], [0, 1] * 30, "alt", z64_base=5)))
    cases.append(("three-types", bind([THREE, every_opcode(False), NONSSA], [0, 1, 2, 2, 1, 0] * 7, "alt")))
    cases.append(("every-opcode", bind([every_opcode(False)], [0, 0], "none")))
    cases.append(("every-opcode-garbage", bind([every_opcode(True)], [0, 0, 0], "alt", z64_base=2, gf2_base=1)))
    cases.append(("non-ssa", bind([NONSSA], [0] * 3, "all")))
    for mode in ("all", "none", "alt"):
        cases.append((f"ports-{mode}", bind([THREE, ZTHREE, ONE], [0, 1, 2, 1, 0] * 3, mode, head=_filler(3), gf2_base=3, z64_base=1)))
    cases.append(("bases", bind([THREE, ZTHREE], [1, 0, 0, 1], "all", z64_base=1000, gf2_base=(1 << 32) - 1 - 6)))
    # about 40 records: every range of it is emitted
    cases.append(("forty", bind([THREE, ZTHREE, EMPTY_WIDE, NONSSA], [0, 2, 1, 3, 2, 2, 0, 1, 3, 3], "alt", head=_filler(5), tail=_filler(5, 1), gf2_base=3)))
    return cases


def bad_cases():
    """[(name, Spec, code)]: a case per code, then the order between two errors"""
    hint = ([GF2.Input(0), SizeHint(1, 1)], (1, 1))
    res = ([GF2.Input(0), _garbage(GF2.Input(1), reserved=1)], (0, 2))
    oob_after = ([GF2.Input(0), GF2.Input(1), GF2.Input(2), GF2.Add(3, 0, 1)], (0, 3))  # record 3
    far = B2A(0, (1 << 32) - 32)  # a + 64 is above 2^32
    cases = [
        ("block-of", Spec([THREE], [0, 1], [WITNESS] * 4), ARG),
        ("bindings-short", Spec([THREE], [0, 0], [WITNESS] * 3), ARG),
        ("bindings-long", Spec([THREE], [0], [WITNESS] * 3), ARG),
        ("bindings-without-instances", Spec([THREE], [], [WITNESS]), ARG),
        ("stated-count", Spec([([], (0, (1 << 32) + 1))]), ARG),
        ("block-reserved", Spec([res]), BAD),
        ("block-opcode", Spec([([_garbage(Z64.Input(0), opcode=10)], (1, 0))]), BAD),
        ("block-domain", Spec([([_garbage(GF2.Input(0), domain=4)], (0, 1))]), BAD),
        ("block-sizehint", Spec([hint]), UNSUPPORTED),
        ("block-dst", Spec([([GF2.Input(1)], (5, 1))]), OOB),
        ("block-a", Spec([([Z64.AssertZero(2)], (2, 5))]), OOB),
        ("block-b", Spec([([GF2.Add(0, 0, 1)], (0, 1))]), OOB),
        ("block-b2a-dst", Spec([([B2A(1, 0)], (1, 64))]), OOB),
        ("block-b2a-a", Spec([([B2A(0, 1)], (1, 64))]), OOB),
        ("head", Spec([THREE], head=[GF2.Input(0), _garbage(GF2.Input(1), reserved=0x100)]), BAD),
        ("tail", Spec([THREE], tail=[_garbage(GF2.Input(1), domain=9)]), BAD),
        ("binding-gf2", Spec([THREE], [0], [WITNESS, 3]), OOB),
        ("binding-z64", Spec([ZTHREE, THREE], [1, 0], [0, 1, 2, 3]), OOB),  # (3 is a GF(2) index: the Z64 count is 3)
        ("base-gf2", Spec([THREE], [0, 0], [WITNESS] * 4, gf2_base=(1 << 32) - 6), UNSUPPORTED),
        ("base-z64", Spec([ZTHREE], [0], [WITNESS] * 2, z64_base=1 << 32), UNSUPPORTED),
        ("head-b2a-above-2^32", Spec([THREE], head=[far]), UNSUPPORTED),
        # the order between two errors
        ("order-earlier-block-first", Spec([oob_after, res]), OOB),
        ("order-earlier-record-first", Spec([([SizeHint(0, 0), _garbage(GF2.Input(0), reserved=1)], (0, 1))]), UNSUPPORTED),
        ("order-inside-a-record", Spec([([_garbage(GF2.Input(7), reserved=1)], (0, 1))]), BAD),
        ("order-block-before-head", Spec([hint], head=[_garbage(GF2.Input(1), reserved=1)]), UNSUPPORTED),
        ("order-head-before-tail-and-instances", Spec([THREE], [5], head=[_garbage(GF2.Input(1), reserved=1)], tail=[far]), BAD),
        ("order-tail-before-instances", Spec([THREE], [5], tail=[_garbage(GF2.Input(1), reserved=1)]), BAD),
        ("order-instances-before-wire-counts", Spec([THREE], [0, 1], [WITNESS] * 2, head=[far]), ARG),
        ("order-binding-count-before-wire-counts", Spec([THREE], [0], [WITNESS], gf2_base=1 << 32), ARG),
        ("order-wire-counts-before-bindings", Spec([THREE], [0], [WITNESS, 1 << 31], gf2_base=1 << 32), UNSUPPORTED),
        ("order-block-before-bindings", Spec([THREE, ([GF2.Input(1)], (0, 1))], [0], [WITNESS, 99]), OOB),
    ]
    for name, s, code in cases:
        assert check(s)[0] == code, (name, check(s)[0])
    return cases


def to_netlist(s: Spec, device_tables=None, device_blocks=None):
    """the Spec through the public interface: reverie_amd.link.Netlist.from_arrays (device_*: a torch device for that side)"""
    from reverie_amd.link import Block, Netlist

    block_of, bindings = s.block_of, s.bindings
    if device_tables is not None:
        import torch

        block_of = torch.from_numpy(block_of.view(np.int32)).to(device_tables)
        bindings = torch.from_numpy(bindings.view(np.int32)).to(device_tables)
    blocks = []
    for o, w in s.blocks:
        if device_blocks is not None:
            import torch

            t = torch.from_numpy(np.frombuffer(o.tobytes(), np.uint8).copy().reshape(-1, 24)).to(device_blocks)
            blocks.append(Block(t, w, n_ports=int(np.count_nonzero(is_input(o)))))
        else:
            blocks.append(Block(o, w))
    return Netlist.from_arrays(blocks, block_of, bindings, s.head, s.tail, s.z64_base, s.gf2_base)


def adder_chain(n=8, seed=5, device=False):
    """-> (Netlist, the last instance's outputs, tail, witness bits, the sum): instance k adds a witness word to instance k - 1's outputs; the head holds nothing, the
    tail asserts the last sum against a constant (tail(value) gives it).  device: the block is parsed on the GPU and stays there"""
    from reverie_amd.link import WITNESS, Block, Netlist
    from reverie_amd.ops import GF2

    rng = np.random.default_rng(seed)
    words = [int(w) for w in rng.integers(0, 1 << 63, n + 1, dtype=np.uint64)]
    adder = Block.from_bristol(bristol_gen.adder64(), device=device)
    assert adder.n_ports == 128 and len(adder.outputs) == 64
    nl = Netlist([adder])
    prev = nl.add(0, [WITNESS] * 128)
    for _ in range(n - 1):
        prev = nl.add(0, prev.outputs + [WITNESS] * 64)
    total = sum(words) % (1 << 64)

    def tail(value):
        w = nl.gf2_base + n * adder.wire_counts[1]
        ops = []
        for k, o in enumerate(prev.outputs):
            ops += [GF2.AddConst(w, o, (value >> k) & 1), GF2.AssertZero(w)]
        return ops

    bits = [(words[0] >> k) & 1 for k in range(64)]
    for wd in words[1:]:
        bits += [(wd >> k) & 1 for k in range(64)]
    return nl, prev.outputs, tail, bits, total


def to_file(s: Spec) -> bytes:
    """the Spec as tests/link_model.cpp reads it"""
    out = struct.pack("<7Q", len(s.blocks), len(s.block_of), len(s.bindings), s.z64_base, s.gf2_base, len(s.head), len(s.tail))
    for o, w in s.blocks:
        out += struct.pack("<3Q", len(o), w[0], w[1]) + o.tobytes()
    return out + s.block_of.tobytes() + s.bindings.tobytes() + s.head.tobytes() + s.tail.tobytes()


def fnv(data: bytes) -> int:
    h = 0xCBF29CE484222325
    for b in data:
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h
