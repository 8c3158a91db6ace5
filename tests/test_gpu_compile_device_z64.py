"""The device compiler on Z64 and mixed GF(2) / Z64 programs (RV_COMPILE_DEVICE | RV_COMPILE_DEVICE_Z64, csrc/compile_dev.hip):
the host compiler's Compiled field by field for whole programs and for a stream's pieces, the host compiler's status and result on
what the device path still hands back, byte-identical proofs and equal answers, and the streams (prover, verifier, evaluator,
batches; host arrays and torch GPU tensors) with Z64 and mixed pieces compiled on the GPU.  Every case compares against the host
path, rv_prove or the oracle, never against the device path itself."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from reverie_amd.ops import B2A, GF2, OP_DTYPE, SizeHint, Z64, program

pytestmark = pytest.mark.gpu

RV_COMPILE_WHOLE_PROVER, RV_COMPILE_KEEP_WIRES, RV_COMPILE_DEVICE, RV_COMPILE_DEVICE_Z64 = 1, 2, 4, 8
DEVZ = RV_COMPILE_DEVICE | RV_COMPILE_DEVICE_Z64
RV_E_ARG = 9
META = json.load(open(os.path.join(GOLDEN, "proofs.json")))
# the tile sizes of compile_dev.hip's kernels: one workgroup (TB) and one scan / radix-sort tile (TILE = TB x 8 items per thread)
WORKGROUP, SCAN_TILE = 256, 2048
EDGE_COUNTS = [WORKGROUP - 1, WORKGROUP + 1, SCAN_TILE - 1, SCAN_TILE + 1]
WIRE_COUNTS = [3, 63, 64, 65, 255, 256, 257, 600, 70000]  # (70 000: a second and a third pass of the 8-bit radix sort)
PROPORTIONS = [1.0, 0.0, 0.1, 0.5, 0.9]  # Z64 share of the ops: pure Z64, pure GF(2), mixtures
M64 = (1 << 64) - 1


def _L():
    from reverie_amd import _lib

    return _lib.lib()


def _ctx():
    import reverie_amd

    return reverie_amd.Context.default()


def _p(prog):
    return prog.ctypes.data_as(C.c_void_p) if len(prog) else None


def compare(prog, wc, flags):
    """-> (host status, path, diff) of rv_hook_compile_compare_device"""
    path, diff = C.c_int(-1), C.c_int(-1)
    rc = _L().rv_hook_compile_compare_device(_ctx().handle, _p(prog), C.c_size_t(len(prog)), C.c_size_t(wc[0]), C.c_size_t(wc[1]), C.c_uint32(flags),
                                             C.byref(path), C.byref(diff))
    return rc, path.value, diff.value


def compare_chunk(prog, wc, start, flags=DEVZ):
    """-> (host status, path, diff) of rv_hook_compile_compare_device_chunk_ex; start = (mask_phase, mask64_phase, on0, pre0, on64, pre64)"""
    prog = np.ascontiguousarray(prog)
    path, diff = C.c_int(-1), C.c_int(-1)
    rc = _L().rv_hook_compile_compare_device_chunk_ex(_ctx().handle, _p(prog), len(prog), wc[0], wc[1], (C.c_uint64 * 6)(*[int(x) for x in start]),
                                                      C.c_uint32(flags), C.byref(path), C.byref(diff))
    return rc, path.value, diff.value


def start_after(prefix):
    """the ChunkStart of the piece that follows `prefix` (no B2A): ShareGen calls of both domains, transcript rows and words"""
    dom, opc = prefix["domain"], prefix["opcode"]
    n = {(d, k): int(((dom == d) & (opc == k)).sum()) for d in (0, 1) for k in (0, 1, 6, 8)}
    m2 = n[0, 0] + n[0, 1] + 2 * n[0, 6]
    m64 = n[1, 0] + n[1, 1] + 2 * n[1, 6]
    return (m2 % 128, m64 % 2, n[0, 0] + n[0, 6] + n[0, 8], n[0, 6], n[1, 0] + 8 * (n[1, 6] + n[1, 8]), n[1, 6])


def lazy_forms_pay(levels, gates):  # compile.h
    return gates > 0 and levels > 64 and gates // levels < 256 and gates < 5000000


def k1_final(prog, wc, monkeypatch):
    """True when the K = 1 compile of the program is the host compiler's final answer (tests/test_gpu_compile_device.py's rule: the
    level count is both domains', the gate count the GF(2) gates')"""
    from reverie_amd import _lib

    info = _lib.CircuitInfo()
    with monkeypatch.context() as m:
        m.setenv("RV_LAZY_K", "1")
        assert _L().rv_hook_compile_info(_p(prog), C.c_size_t(len(prog)), C.c_size_t(wc[0]), C.c_size_t(wc[1]), C.c_uint32(0), C.c_size_t(0),
                                         C.byref(info)) == 0
    gates = info.gf2_inputs + info.gf2_muls + info.gf2_asserts + info.gf2_linear
    return not lazy_forms_pay(info.levels, gates)


# ---- the generator (circuits.random_mixed emits B2A) ----
def gen_mixed(rng, n_ops, w64, w2, z_share, valid=False, hints=True, randoms=True):
    """A program over all ten opcodes of both domains with heavy wire reuse: reads of never-written wires, Mul(d, a, a), ops whose
    dst is one of their operands, AssertZero on fresh and on stale wires, SizeHints that grow nothing.  valid: the witness satisfies
    every AssertZero (they sit on wires whose value is known to be zero) -- for proofs.  randoms=False: Const ops in place of the Random
    ops (cleartext evaluation takes no Random).  -> (program, GF(2) witness, Z64 witness)"""
    ops, wit2, wit64 = [], [], []
    val = ({}, {})  # wire -> value (missing: never written = 0; None: differs between repetitions, a Random op's)
    zeros = ([], [])  # wires that held a zero when last looked at: the stale AssertZero targets
    hot = (min(w2, 12), min(w64, 12))

    def wire(d):
        W = w64 if d else w2
        return int(rng.integers(0, hot[d])) if rng.random() < 0.7 else int(rng.integers(0, W))

    def get(d, w):
        return val[d].get(w, 0)

    def put(d, w, v):
        val[d][w] = v
        if v == 0:
            zeros[d].append(w)

    for _ in range(n_ops):
        d = 1 if rng.random() < z_share else 0
        if (d and w64 == 0) or (not d and w2 == 0):
            d ^= 1
        O = Z64 if d else GF2
        mod = (lambda x: x & M64) if d else (lambda x: x & 1)
        if hints and rng.random() < 0.02:
            ops.append(SizeHint(int(rng.integers(0, w64 + 1)), int(rng.integers(0, w2 + 1))))
            continue
        k = int(rng.choice(10, p=[0.08, 0.04, 0.16, 0.08, 0.12, 0.07, 0.22, 0.07, 0.08, 0.08]))
        if k == 1 and not randoms:
            k = 9
        dst, a, b = wire(d), wire(d), wire(d)
        r = rng.random()
        if r < 0.1:
            b = a  # Mul(d, a, a), Add(d, a, a), Sub(d, a, a)
        elif r < 0.25:
            dst = a  # the op overwrites its own operand
        va, vb = get(d, a), get(d, b)
        c = int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2)) if d else int(rng.integers(0, 2))
        both = None if va is None or vb is None else (va, vb)
        if k == 0:
            v = int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2)) if d else int(rng.integers(0, 2))
            (wit64 if d else wit2).append(v)
            ops.append(O.Input(dst))
            put(d, dst, v)
        elif k == 1:
            ops.append(O.Random(dst))
            put(d, dst, None)
        elif k == 2:
            ops.append(O.Add(dst, a, b))
            put(d, dst, None if both is None else mod(va + vb))
        elif k == 3:
            ops.append(O.AddConst(dst, a, c))
            put(d, dst, None if va is None else mod(va + c))
        elif k == 4:
            ops.append(O.Sub(dst, a, b))
            put(d, dst, None if both is None else mod(va - vb))
        elif k == 5:
            ops.append(O.SubConst(dst, a, c))
            put(d, dst, None if va is None else mod(va - c))
        elif k == 6:
            ops.append(O.Mul(dst, a, b))
            put(d, dst, None if both is None else mod(va * vb))
        elif k == 7:
            if rng.random() < 0.3:
                c = 0
            ops.append(O.MulConst(dst, a, c))
            put(d, dst, None if va is None else mod(va * c))
        elif k == 9:
            if rng.random() < 0.3:
                c = 0
            ops.append(O.Const(dst, c))
            put(d, dst, mod(c))
        else:  # AssertZero
            if not valid:
                ops.append(O.AssertZero(a))
                continue
            cand = [w for w in zeros[d][-8:] + zeros[d][:2] if get(d, w) == 0]
            if cand and rng.random() < 0.7:
                ops.append(O.AssertZero(cand[int(rng.integers(0, len(cand)))]))  # a stale zero (or a never-written wire below)
            elif get(d, a) == 0:
                ops.append(O.AssertZero(a))
            elif va is not None:
                ops.append(O.SubConst(dst, a, va))  # a fresh zero
                ops.append(O.AssertZero(dst))
                put(d, dst, 0)
    return program(ops), wit2, wit64


def z_chain(depth, w=0):
    return [Z64.Input(w)] + [Z64.AddConst(w, w, 3) if i % 2 else Z64.Mul(w, w, w) for i in range(depth)]


def g_chain(depth, w=0):
    return [GF2.Input(w), GF2.Input(w + 1)] + [GF2.Mul(w, w, w + 1) for _ in range(depth)]


def shaped_programs():
    """(name, program, wire counts): the op counts around one workgroup and one scan tile, pure Z64 (every op is a Z64 gate) and
    mixed; a Z64 chain deeper than the GF(2) part and the reverse (each domain's tables end in empty levels once); a chain deeper
    than the first batches of rounds"""
    rng = np.random.default_rng(0x264)
    out = []
    for n in EDGE_COUNTS + [WORKGROUP, SCAN_TILE]:
        out.append(("pure_z64_%d" % n, gen_mixed(rng, n, 40, 0, 1.0, hints=False)[0][:n], (40, 0)))
        out.append(("mixed_%d" % n, gen_mixed(rng, n, 300, 300, 0.5)[0][:n], (300, 300)))
    out.append(("z64_deeper", program(z_chain(40) + g_chain(3) + [Z64.AssertZero(0), GF2.AssertZero(0)]), (2, 2)))
    out.append(("gf2_deeper", program(g_chain(40) + z_chain(3) + [Z64.AssertZero(0), GF2.AssertZero(0)]), (2, 2)))
    out.append(("z64_chain_300", program(z_chain(300) + g_chain(2)), (1, 2)))
    out.append(("both_chains_300", program([op for pair in zip(z_chain(300), g_chain(299)) for op in pair]), (1, 2)))
    return out


_PROGRAMS = []


def programs():
    """every wire count with every proportion; op counts 20 - 4 000"""
    if not _PROGRAMS:
        rng = np.random.default_rng(0x2640)
        sizes = [20, 120, 400, 1500, 4000]
        k = 0
        for w in WIRE_COUNTS:
            for share in PROPORTIONS:
                n = sizes[k % len(sizes)]
                k += 1
                w2 = w if share < 1.0 else int(rng.choice([0, 5]))
                w64 = w if share > 0.0 else int(rng.choice([0, 5]))
                prog, _, _ = gen_mixed(rng, n, w64, w2, share)
                _PROGRAMS.append(("w%d_z%.1f_n%d" % (w, share, n), prog, (w64, w2), share))
        _PROGRAMS.extend((name, prog, wc, None) for name, prog, wc in shaped_programs())
    return _PROGRAMS


HAND = {
    "swap_z64": ([Z64.AddConst(5, 0, 0), Z64.AddConst(0, 1, 0), Z64.AddConst(1, 5, 0), GF2.AddConst(5, 0, 0), GF2.AddConst(0, 1, 0), GF2.AddConst(1, 5, 0)], (8, 8)),
    "mul_assert": ([Z64.Input(0), GF2.Input(0), Z64.Mul(1, 0, 2), Z64.Mul(1, 1, 1), GF2.Mul(1, 0, 0), Z64.AssertZero(3), Z64.Sub(3, 1, 1), Z64.AssertZero(3),
                    GF2.AssertZero(2), Z64.Random(2), Z64.Add(2, 2, 0), SizeHint(4, 4), Z64.Const(0, 7), Z64.MulConst(3, 0, 3), Z64.SubConst(3, 3, 21),
                    Z64.AssertZero(3)], (4, 4)),
    "gf2_then_z64": ([GF2.Input(0), GF2.Input(1), GF2.Mul(2, 0, 1), GF2.Add(3, 2, 0), GF2.AssertZero(5), Z64.Input(0), Z64.AssertZero(1), Z64.Input(0),
                      Z64.Mul(1, 0, 0), Z64.AddConst(1, 1, 1)], (2, 6)),
}


# ---- 1. whole programs ----
def test_whole_programs_forced_form():
    for name, prog, wc, _ in programs():
        assert compare(prog, wc, DEVZ | RV_COMPILE_WHOLE_PROVER) == (0, 1, 0), name
    for name, (ops, wc) in HAND.items():
        assert compare(program(ops), wc, DEVZ | RV_COMPILE_WHOLE_PROVER) == (0, 1, 0), name


def test_whole_programs_plain_form(monkeypatch):
    n_dev = 0
    for name, prog, wc, share in programs():
        rc, path, diff = compare(prog, wc, DEVZ)
        assert (rc, diff) == (0, 0), (name, rc, path, diff)
        want = 1 if share == 1.0 or name.startswith("pure_z64") else (1 if k1_final(prog, wc, monkeypatch) else 0)
        assert path == want, (name, path, want)
        n_dev += path
    # (every pure-Z64 program at least: heavy wire reuse makes most of the others deep and narrow, which the host compiler recompiles)
    assert n_dev >= sum(1 for name, _, _, share in programs() if share == 1.0 or name.startswith("pure_z64")), n_dev


# ---- 2. chunks ----
def test_chunks_of_the_programs():
    rng = np.random.default_rng(0x2641)
    for name, prog, wc, _ in programs():
        cuts = sorted(set(int(c) for c in rng.integers(0, len(prog) + 1, 3)))
        edges = [0] + cuts + [len(prog)]
        for a, b in zip(edges[:-1], edges[1:]):  # (a == b: an empty piece)
            for start in (start_after(prog[:a]), (int(rng.integers(0, 128)), int(rng.integers(0, 2)), 5, 3, 17, 2)):
                assert compare_chunk(prog[a:b], wc, start) == (0, 1, 0), (name, a, b, start)


def test_chunks_hand_written_cut_at_every_op():
    phases, n_empty = set(), 0
    for name, (ops, wc) in HAND.items():
        prog = program(ops)
        for a in range(len(prog) + 1):
            for b in (a, a + 1, min(a + 3, len(prog)), len(prog)):
                if b > len(prog):
                    continue
                start = start_after(prog[:a])
                phases.add(start[1])
                n_empty += a == b
                assert compare_chunk(prog[a:b], wc, start) == (0, 1, 0), (name, a, b, start)
    assert phases == {0, 1} and n_empty > 0
    # a piece that writes no Z64 wire (its Z64 side is AssertZero ops only), one that swaps two Z64 wires, an empty one: at both phases
    no_write = program([Z64.AssertZero(0), Z64.AssertZero(2), GF2.Input(0)])
    swap = program(HAND["swap_z64"][0][:3])
    for start in [(0, 0, 0, 0, 0, 0), (127, 1, 5, 3, 9, 1)]:
        assert compare_chunk(no_write, (3, 3), start) == (0, 1, 0)
        assert compare_chunk(swap, (8, 0), start) == (0, 1, 0)
        assert compare_chunk(swap, (8, 8), start) == (0, 1, 0)
        assert compare_chunk(np.zeros(0, OP_DTYPE), (8, 8), start) == (0, 1, 0)


# ---- 3. scope ----
def _compile_status(prog, wc, **kw):
    import reverie_amd

    try:
        c = reverie_amd.Circuit(prog, wc, **kw)
    except reverie_amd.ReverieError as e:
        return e.code, None, None
    info, on_dev = c.info, c.compiled_on_device
    c.close()
    return 0, {k: v for k, v in info.items() if k not in ("compile_us", "upload_us")}, on_dev


def test_scope_fallbacks_match_host():
    zbase = [Z64.Input(0), Z64.Input(1), Z64.Mul(2, 0, 1), GF2.Input(0)]
    bad_opcode = program(zbase + [Z64.Add(1, 0, 0)])
    bad_opcode["opcode"][4] = 42
    reserved = program(zbase + [Z64.Add(1, 0, 0)])
    reserved["reserved"][4] = 1
    cases = {
        "b2a": (program([GF2.Input(i) for i in range(64)] + [B2A(0, 0), Z64.AddConst(1, 0, 5)]), (2, 64), 0),
        "sizehint_grows_z64": (program(zbase + [SizeHint(9, 1), Z64.Input(8)]), (3, 1), 0),
        "sizehint_grows_gf2": (program(zbase + [SizeHint(3, 2), GF2.Input(1)]), (3, 1), 0),
        "z64_wire_oob": (program(zbase + [Z64.Add(1, 0, 3)]), (3, 1), 3),
        "z64_dst_oob": (program(zbase + [Z64.Const(3, 1)]), (3, 1), 3),
        "z64_assert_oob": (program(zbase + [Z64.AssertZero(3)]), (3, 1), 3),
        "bad_z64_opcode": (bad_opcode, (3, 1), 5),
        "reserved": (reserved, (3, 1), 5),
    }
    for name, (prog, wc, want_rc) in cases.items():
        for flags in (DEVZ, DEVZ | RV_COMPILE_WHOLE_PROVER):
            rc, path, diff = compare(prog, wc, flags)
            assert (rc, path, diff) == (want_rc, 0, 0), (name, flags, rc, path, diff)
        want = _compile_status(prog, wc)
        assert want[0] == want_rc, name
        got = _compile_status(prog, wc, device_compile=True, device_z64=True)
        assert got[:2] == want[:2] and not got[2], name
    # the same in a chunk (a SizeHint that grows a wire count is an error there)
    for name in ("b2a", "z64_wire_oob", "bad_z64_opcode", "reserved", "sizehint_grows_z64"):
        prog, wc, want_rc = cases[name]
        rc, path, diff = compare_chunk(prog, wc, (3, 1, 7, 2, 8, 1))
        assert (path, diff) == (0, 0) and (rc == want_rc if want_rc else True), (name, rc, path, diff)
    assert compare_chunk(cases["sizehint_grows_z64"][0], (3, 1), (0, 0, 0, 0, 0, 0))[0] == 8
    # KEEP_WIRES stays the host compiler's
    prog, _, _ = gen_mixed(np.random.default_rng(3), 300, 20, 20, 0.5)
    assert compare(prog, (20, 20), DEVZ | RV_COMPILE_KEEP_WIRES) == (0, 0, 0)
    got = _compile_status(prog, (20, 20), device_compile=True, device_z64=True, keep_wires=True)
    assert got[:2] == _compile_status(prog, (20, 20), keep_wires=True)[:2] and not got[2]
    assert _compile_status(prog, (20, 20), device_compile=True, device_z64=True)[2]


def test_old_flags_keep_their_scope():
    """the two Z64 programs of tests/test_gpu_compile_device.py, and Z64 pieces, under every flag value that existed before"""
    z1 = program([Z64.Input(0), Z64.Input(1), Z64.Mul(2, 0, 1), GF2.Input(0)])
    z2 = program([Z64.Input(0), Z64.Input(1), Z64.Mul(2, 0, 1), GF2.Input(0), GF2.Mul(1, 0, 0)])
    for prog, wc in ((z1, (3, 1)), (z2, (3, 2))):
        for flags in (0, RV_COMPILE_DEVICE, RV_COMPILE_DEVICE | RV_COMPILE_WHOLE_PROVER):
            assert compare(prog, wc, flags) == (0, 0, 0), flags
        assert compare(prog, wc, DEVZ) == (0, 1, 0)
        assert not _compile_status(prog, wc, device_compile=True)[2]
        for flags in (0, RV_COMPILE_DEVICE):
            assert compare_chunk(prog, wc, (0, 0, 0, 0, 0, 0), flags) == (0, 0, 0)
        assert compare_chunk(prog, wc, (0, 0, 0, 0, 0, 0)) == (0, 1, 0)
    hinted = program([GF2.Input(0), SizeHint(0, 1), GF2.Mul(1, 0, 0)])
    assert compare(hinted, (0, 2), RV_COMPILE_DEVICE) == (0, 0, 0)
    assert compare(hinted, (0, 2), DEVZ) == (0, 1, 0)


def test_the_bit_alone_is_an_argument_error():
    import reverie_amd

    L, ctx = _L(), _ctx()
    prog = program([Z64.Input(0), GF2.Input(0)])
    start = (C.c_uint64 * 6)()
    path, diff, h = C.c_int(), C.c_int(), C.c_void_p()
    for flags in (RV_COMPILE_DEVICE_Z64, RV_COMPILE_DEVICE_Z64 | RV_COMPILE_WHOLE_PROVER):
        assert L.rv_circuit_compile_ex(ctx.handle, _p(prog), C.c_size_t(2), C.c_size_t(1), C.c_size_t(1), C.c_uint32(flags), C.byref(h)) == RV_E_ARG
        assert L.rv_hook_compile_compare_device(ctx.handle, _p(prog), 2, 1, 1, flags, C.byref(path), C.byref(diff)) == RV_E_ARG
    assert L.rv_ctx_set_compile_flags(ctx.handle, RV_COMPILE_DEVICE_Z64) == RV_E_ARG
    assert L.rv_hook_compile_compare_device_chunk_ex(ctx.handle, _p(prog), 2, 1, 1, start, RV_COMPILE_DEVICE_Z64, C.byref(path), C.byref(diff)) == RV_E_ARG
    from reverie_amd.stream import StreamingEvaluator, StreamingProver

    sp, se = StreamingProver((1, 1)), StreamingEvaluator((1, 1))
    try:
        assert L.rv_stream_set_compile_flags(sp.handle, RV_COMPILE_DEVICE_Z64) == RV_E_ARG
        assert L.rv_eval_stream_set_compile_flags(se.handle, RV_COMPILE_DEVICE_Z64) == RV_E_ARG
        assert L.rv_stream_set_compile_flags(sp.handle, DEVZ) == 0
        assert L.rv_eval_stream_set_compile_flags(se.handle, DEVZ) == 0
    finally:
        sp.close()
        se.close()
    # rv_circuit_compile_device implies RV_COMPILE_DEVICE; the context takes both bits together
    ctx2 = reverie_amd.Context(0)
    ctx2.set_compile_flags(DEVZ)
    ctx2.set_compile_flags(0)
    ctx2.close()
    with pytest.raises(ValueError):
        reverie_amd.Circuit(prog, (1, 1), device_z64=True)
    assert L.rv_abi_version() == 8


# ---- 4. proofs and answers ----
def _no_times(info):
    return {k: v for k, v in info.items() if k not in ("compile_us", "upload_us")}


def proof_programs():
    m = META["z64_mix"]
    out = [("z64_mix", program([tuple(o) for o in m["ops"]]), m["wit_gf2"], [int(x) for x in m["wit_z64"]], tuple(m["wire_counts"]))]
    rng = np.random.default_rng(0x2642)
    for k, (n, w64, w2, share) in enumerate([(300, 9, 9, 0.5), (1600, 40, 300, 0.9), (500, 64, 5, 1.0), (700, 257, 65, 0.1)]):
        prog, w2v, w64v = gen_mixed(rng, n, w64, w2, share, valid=True, randoms=k % 2 == 0)  # (gen1, gen3: evaluated in the clear too)
        out.append(("gen%d" % k, prog, w2v, w64v, (w64, w2)))
    return out


def _evaluate(c, w2, w64):
    import reverie_amd

    try:
        e = c.evaluate(w2, w64)
    except reverie_amd.ReverieError as err:
        return ("error", err.code, None)
    return (bool(e.ok), int(e.n_failed), e.first_failed_op)


def test_proofs_and_answers(oracle, rule_seeds):
    import torch

    import reverie_amd

    for k, (name, prog, w2, w64, wc) in enumerate(proof_programs()):
        # the plain form where it is the host compiler's final answer; a deep, narrow program (heavy wire reuse makes some) in the forced
        # lazy-sum form, which is final for every program: the device compiler makes the circuit either way, and the proof bytes do not
        # depend on the form
        wp = compare(prog, wc, DEVZ)[1] == 0
        assert compare(prog, wc, DEVZ | (RV_COMPILE_WHOLE_PROVER if wp else 0)) == (0, 1, 0), name
        plain = reverie_amd.Circuit(prog, wc)
        host = reverie_amd.Circuit(prog, wc, whole_prover=True) if wp else plain
        dev = reverie_amd.Circuit(prog, wc, whole_prover=wp, device_compile=True, device_z64=True)
        t = torch.from_numpy(prog.view(np.uint8).reshape(len(prog), 24).copy()).cuda()
        dten = reverie_amd.Circuit.from_device_ops(t, wc, whole_prover=wp, device_z64=True)
        assert bytes(reverie_amd.Proof.new(plain, w2, w64, seeds=rule_seeds)) == bytes(reverie_amd.Proof.new(host, w2, w64, seeds=rule_seeds)), name
        assert not host.compiled_on_device and dev.compiled_on_device and dten.compiled_on_device, name
        assert _no_times(dev.info) == _no_times(host.info) == _no_times(dten.info), name
        ph = reverie_amd.Proof.new(host, w2, w64, seeds=rule_seeds)
        want = bytes(ph)
        for c in (dev, dten):
            p = reverie_amd.Proof.new(c, w2, w64, seeds=rule_seeds)
            assert bytes(p) == want, name
            assert p.verify(host, strict=True) and ph.verify(c, strict=True), name
        if k in (1, 3):
            assert want == oracle.prove(prog, w2, w64, wc, rule_seeds), name
        # rv_evaluate: the same status from all three (a program with Random ops: the same refusal); a wrong witness fails the same
        # AssertZero
        eh = _evaluate(host, w2, w64)
        has_random = bool(((prog["opcode"] == 1) & (prog["domain"] < 2)).any())
        assert eh == ((("error", 8, None)) if has_random else (True, 0, None)), (name, eh)
        for wz in [w64] + ([[(w64[0] + 1) & M64] + list(w64[1:])] if w64 else []):
            eh = _evaluate(host, w2, wz)
            assert _evaluate(dev, w2, wz) == eh and _evaluate(dten, w2, wz) == eh, name
        for c in {plain, host, dev, dten}:
            c.close()


def test_prove_ops_under_context_flag(rule_seeds):
    import reverie_amd

    name, prog, w2, w64, wc = proof_programs()[2]
    assert len(prog) >= 1024  # (shorter programs bypass the ops cache)
    plain, flagged = reverie_amd.Context(0), reverie_amd.Context(0)
    flagged.set_compile_flags(DEVZ)
    want = bytes(reverie_amd.Proof.new(prog, w2, w64, wc, seeds=rule_seeds, ctx=plain))
    for _ in range(2):  # cold, then from the ops cache
        got = reverie_amd.Proof.new(prog, w2, w64, wc, seeds=rule_seeds, ctx=flagged)
        assert bytes(got) == want
        assert got.verify(prog, wc, ctx=flagged, strict=True)
    flagged.set_compile_flags(0)
    assert bytes(reverie_amd.Proof.new(prog, w2, w64, wc, seeds=rule_seeds, ctx=flagged)) == want
    plain.close()
    flagged.close()


# ---- 5. streams ----
def device_chunks():
    return int(_L().rv_hook_stream_device_chunks())


def _edges(prog, cuts):
    e = [0] + sorted(set(int(c) for c in cuts if 0 < c < len(prog))) + [len(prog)]
    return list(zip(e[:-1], e[1:]))


def _pieces(prog, w2, w64, cuts):
    """split (prog, witness) at the op indices `cuts`: every piece gets the witness elements its Input gates consume"""
    out = []
    i2 = i64 = 0
    for a, b in _edges(prog, cuts):
        part = prog[a:b]
        n2 = int(((part["domain"] == 0) & (part["opcode"] == 0)).sum())
        n64 = int(((part["domain"] == 1) & (part["opcode"] == 0)).sum())
        out.append((part, list(w2[i2:i2 + n2]), list(w64[i64:i64 + n64])))
        i2 += n2
        i64 += n64
    return out


def _no_b2a(part):
    return len(part) > 0 and not bool((part["domain"] == 2).any())


def _tensor(part):
    import torch

    return torch.from_numpy(np.ascontiguousarray(part).view(np.uint8).reshape(len(part), 24).copy()).cuda()


def _stream(prog, w2, w64, wc, seeds, cuts1, cuts2=None, same_cuts=False, on_gpu=False, **kw):
    from reverie_amd.stream import StreamingProver

    sp = StreamingProver(wc, seeds=seeds, device_compile=True, device_z64=True, **kw)
    try:
        if same_cuts:
            sp.same_cuts()
        for part, a, b in _pieces(prog, w2, w64, cuts1):
            sp.feed(_tensor(part) if on_gpu else part, a, b)
        comm = sp.commit()
        for part, a, b in _pieces(prog, w2, w64, cuts1 if cuts2 is None else cuts2):
            sp.feed(_tensor(part) if on_gpu else part, a, b)
        proof = sp.finish()
    finally:
        sp.close()
    assert proof.comm == comm
    return proof


_STREAM_PROGRAMS = []


def stream_programs():
    if not _STREAM_PROGRAMS:
        rng = np.random.default_rng(0x2643)
        # (a stream cuts a feed into pieces of 1024 ops at least: three or four pieces each; the second one has Random ops)
        for k, (n, w64, w2, share) in enumerate([(2500, 12, 12, 0.5), (3300, 65, 257, 0.9), (2100, 300, 9, 0.1)]):
            prog, w2v, w64v = gen_mixed(rng, n, w64, w2, share, valid=True, randoms=k == 1)
            _STREAM_PROGRAMS.append((prog, w2v, w64v, (w64, w2)))
    return _STREAM_PROGRAMS


@pytest.mark.parametrize("k", range(3))
@pytest.mark.parametrize("on_gpu", [False, True])
def test_stream_prover(rule_seeds, monkeypatch, k, on_gpu):
    import reverie_amd

    prog, w2, w64, wc = stream_programs()[k]
    rng = np.random.default_rng(60 + k)
    want = bytes(reverie_amd.Proof.new(prog, w2, w64, wc, seeds=rule_seeds))
    n = len(prog)
    c1, c2 = rng.integers(1, n, 6), rng.integers(1, n, 7)
    e1, e2 = _edges(prog, c1), _edges(prog, c2)
    before = device_chunks()
    assert bytes(_stream(prog, w2, w64, wc, rule_seeds, c1, c2, on_gpu=on_gpu)) == want
    # (a pass-2 piece with the position and length of a pass-1 piece comes out of pass 1's cache of compiled chunks)
    assert device_chunks() - before == len(e1) + sum(e not in e1 for e in e2)
    for keep_mb in ("0", None):
        if keep_mb is None:
            monkeypatch.delenv("RV_STREAM_KEEP_MB", raising=False)
        else:
            monkeypatch.setenv("RV_STREAM_KEEP_MB", keep_mb)
        before = device_chunks()
        assert bytes(_stream(prog, w2, w64, wc, rule_seeds, c1, same_cuts=True, on_gpu=on_gpu)) == want
        assert device_chunks() - before == len(e1)  # (pass 2: pass 1's compiled chunks, or its kept transcripts)


@pytest.mark.parametrize("k", range(3))
def test_stream_verifier_evaluator_batches(rule_seeds, k):
    import reverie_amd
    from reverie_amd.stream import (StreamingEvaluator, StreamingVerifier, evaluate_streaming, prove_streaming, prove_streaming_batch, verify_streaming,
                                    verify_streaming_batch)

    prog, w2, w64, wc = stream_programs()[k]
    n = len(prog)
    CH = 1024  # (the smallest piece a stream cuts)
    n_pieces = -(-n // CH)
    assert n_pieces >= 3
    has_random = k == 1
    circ = reverie_amd.Circuit(prog, wc, keep_wires=not has_random)
    proof = reverie_amd.Proof.new(circ, w2, w64, seeds=rule_seeds)
    want = bytes(proof)
    ops_host, ops_gpu = prog, _tensor(prog)
    for ops in (ops_host, ops_gpu):
        before = device_chunks()
        got, info = prove_streaming(ops, w2, w64, wc, seeds=rule_seeds, max_chunk_ops=CH, device_compile=True, device_z64=True)
        assert bytes(got) == want and device_chunks() - before == n_pieces
        before = device_chunks()
        ok, _ = verify_streaming(ops, wc, proof, max_chunk_ops=CH, device_compile=True, device_z64=True)
        assert ok and device_chunks() - before == n_pieces
    # the verifier fed in pieces
    cuts = list(range(97, n, 97))
    sv = StreamingVerifier(wc, proof, device_compile=True, device_z64=True)
    before = device_chunks()
    for a, b in _edges(prog, cuts):
        sv.feed(prog[a:b])
    assert sv.finish() and device_chunks() - before == len(_edges(prog, cuts))
    sv.close()
    # the evaluator: batches 1 and 4 (the witness, and three with another first element each: other values, some failing asserts)
    for batch in (1, 4):
        if has_random:  # (cleartext evaluation takes no Random op: the same refusal with the flag as without it)
            for kw in ({}, {"device_compile": True, "device_z64": True}):
                with pytest.raises(reverie_amd.ReverieError) as err:
                    evaluate_streaming(prog, w2, w64, wc, max_chunk_ops=CH, **kw)
                assert err.value.code == 8
            break
        g = np.tile(np.asarray(w2, np.uint8), (batch, 1))
        z = np.tile(np.asarray(w64, np.uint64), (batch, 1))
        for b in range(1, batch):
            if z.shape[1]:
                z[b, 0] += np.uint64(b)
            if g.shape[1]:
                g[b, 0] ^= 1
        ref = circ.evaluate_batch(g, z, values=True) if batch > 1 else None
        for ops in (ops_host, ops_gpu):
            before = device_chunks()
            r = evaluate_streaming(ops, g if batch > 1 else g[0], z if batch > 1 else z[0], wc, max_chunk_ops=CH, values=True, device_compile=True,
                                   device_z64=True)
            assert device_chunks() - before == n_pieces
            plain = evaluate_streaming(prog, g if batch > 1 else g[0], z if batch > 1 else z[0], wc, max_chunk_ops=CH, values=True)
            for x in (plain,) + ((ref,) if ref is not None else ()):
                assert np.array_equal(r.ok, x.ok) and np.array_equal(r.n_failed, x.n_failed) and np.array_equal(r.first_failed_op, x.first_failed_op)
                assert np.array_equal(r.gf2, x.gf2) and np.array_equal(r.z64, x.z64)
            assert bool(r.ok[0])
        se = StreamingEvaluator(wc, batch, device_compile=True, device_z64=True)
        i2 = i64 = 0
        for part, a, b in _pieces(prog, g[0], z[0], cuts):
            se.feed(part, g[:, i2:i2 + len(a)], z[:, i64:i64 + len(b)])
            i2, i64 = i2 + len(a), i64 + len(b)
        rp = se.finish(values=True)
        se.close()
        assert np.array_equal(rp.ok, r.ok) and np.array_equal(rp.gf2, r.gf2) and np.array_equal(rp.z64, r.z64)
    # a batch of 3 witnesses (the same witness under three seed sets: three different proofs)
    seeds3 = np.stack([np.roll(np.asarray(rule_seeds, np.uint8).reshape(256, 16), b, axis=0) for b in range(3)])
    g3, z3 = np.tile(np.asarray(w2, np.uint8), (3, 1)), np.tile(np.asarray(w64, np.uint64), (3, 1))
    wants = [bytes(reverie_amd.Proof.new(circ, w2, w64, seeds=seeds3[b])) for b in range(3)]
    for ops in (ops_host, ops_gpu):
        before = device_chunks()
        proofs = prove_streaming_batch(ops, g3, z3, wc, seeds=seeds3, max_chunk_ops=CH, device_compile=True, device_z64=True)
        assert [bytes(p) for p in proofs] == wants and device_chunks() - before == n_pieces
        before = device_chunks()
        assert verify_streaming_batch(ops, wc, proofs, max_chunk_ops=CH, device_compile=True, device_z64=True) == [True] * 3
        assert device_chunks() - before == n_pieces
    circ.close()


@pytest.mark.parametrize("on_gpu", [False, True])
def test_stream_b2a_piece_in_the_middle(rule_seeds, on_gpu):
    import reverie_amd

    prog, w2, w64, wc = stream_programs()[0]
    half = len(prog) // 2
    # 64 fresh GF(2) wires behind the program's own, bridged into a Z64 wire of its own; the second half runs on
    bridge = program([GF2.Const(wc[1] + i, (0x5A >> (i % 8)) & 1) for i in range(64)] + [B2A(wc[0], wc[1]), Z64.AddConst(wc[0], wc[0], 1)])
    full = np.concatenate([prog[:half], bridge, prog[half:]])
    wcb = (wc[0] + 1, wc[1] + 64)
    want = bytes(reverie_amd.Proof.new(full, w2, w64, wcb, seeds=rule_seeds))
    cuts = [half // 2, half, half + len(bridge), half + len(bridge) + (len(prog) - half) // 2]
    parts = [full[a:b] for a, b in _edges(full, cuts)]
    assert [_no_b2a(p) for p in parts] == [True, True, False, True, True]
    before = device_chunks()
    assert bytes(_stream(full, w2, w64, wcb, rule_seeds, cuts, on_gpu=on_gpu)) == want
    assert device_chunks() - before == 4
    traffic = (C.c_uint64 * 2)()
    assert _L().rv_hook_stream_op_traffic(traffic) == 0
    d2h = int(traffic[1])
    if on_gpu:  # only the B2A piece is copied down (once: pass 2 takes pass 1's compile from the cache), 24 bytes per op
        assert bytes(_stream(full, w2, w64, wcb, rule_seeds, cuts, on_gpu=True)) == want
        assert _L().rv_hook_stream_op_traffic(traffic) == 0
        assert int(traffic[1]) - d2h == 24 * len(bridge)
