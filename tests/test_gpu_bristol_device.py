"""rv_bristol_parse_device against rv_bristol_parse (the definition): the same records byte for byte, the same counts and the same
return code for every text of the shared corpus (bristol_cases.py), from host text and from text in GPU memory; the capacity protocol;
reads that stay inside `len`; a header that claims more than any memory; device-parsed programs through compile, proof and compaction."""
import time

import numpy as np
import pytest

import bristol_cases as bc
import bristol_gen
from reverie_amd.ops import OP_DTYPE

pytestmark = pytest.mark.gpu
REC = OP_DTYPE.itemsize


@pytest.fixture(scope="module")
def rv():
    import reverie_amd

    return reverie_amd


@pytest.fixture(scope="module")
def ctx(rv):
    return rv.Context.default()


@pytest.fixture(scope="module")
def big_texts():
    """[(name, text, fmt)]: adder64 and AES-128 (the slowest to make: once)"""
    return [("adder64", bristol_gen.adder64().encode(), 0), ("aes128", bristol_gen.aes128().encode(), 0)]


def on_gpu(text: bytes, lead=3, tail=b""):
    """(tensor, device address of the text): the text at an odd offset inside a larger GPU allocation, `tail` right behind it"""
    import torch

    whole = b"\n" * lead + text + tail + b"\n2 1 0 1 2 XOR\n"
    t = torch.from_numpy(np.frombuffer(whole, np.uint8).copy()).cuda()
    return t, t.data_ptr() + lead


def parse_both_ways(ctx, text, expected, fmt, want_n):
    """the device parser's answers for host text and for device text: [(rc, n_ops, info, record bytes)]"""
    import torch

    out = []
    keep, addr = on_gpu(text)
    for src, on_dev in ((np.frombuffer(text, np.uint8) if text else np.zeros(1, np.uint8), False), (addr, True)):
        cap = want_n + 2
        d_ops = torch.full((cap, REC), 0xA5, dtype=torch.uint8, device="cuda")
        rc, n, info = bc.device_parse(ctx, src, len(text), on_dev, expected, fmt, d_ops, cap)
        torch.cuda.synchronize()
        recs = d_ops.cpu().numpy().tobytes()
        if rc == 0:
            assert recs[n * REC:] == b"\xA5" * ((cap - n) * REC), "records beyond n_ops were written"
        out.append((rc, n, info, recs[:n * REC]))
    del keep
    return out


def check_parity(ctx, text, fmt):
    rc, n, recs, info = bc.host_parse(text, None, fmt)
    assert rc == 0
    exp = [(7 * k + 1) % 3 % 2 for k in range(info["n_outputs"])]
    for expected in (None, exp):
        rc, n, recs, info = bc.host_parse(text, expected, fmt)
        assert rc == 0
        for got in parse_both_ways(ctx, text, expected, fmt, n):
            assert got[0] == 0
            assert got[1] == n and got[2] == info
            assert got[3] == recs


@pytest.mark.parametrize("name,text,fmt", bc.well_formed(), ids=[c[0] for c in bc.well_formed()])
def test_parity_well_formed(ctx, name, text, fmt):
    check_parity(ctx, text, fmt)


@pytest.mark.parametrize("name,text,fmt", bc.boundary_texts(), ids=[c[0] for c in bc.boundary_texts()])
def test_parity_around_the_tiles(ctx, name, text, fmt):
    check_parity(ctx, text, fmt)


@pytest.mark.parametrize("which", [0, 1], ids=["adder64", "aes128"])
def test_parity_circuits(ctx, big_texts, which):
    check_parity(ctx, big_texts[which][1], 0)


@pytest.mark.parametrize("name,text,expected,fmt,code", bc.error_texts(), ids=[c[0] for c in bc.error_texts()])
def test_error_parity(ctx, name, text, expected, fmt, code):
    assert bc.host_parse(text, expected, fmt)[0] == code
    for rc, n, _, _ in parse_both_ways(ctx, text, expected, fmt, 4096):
        assert rc == code and n == 0
    # a sizing call answers with the text's own code
    assert bc.device_parse(ctx, np.frombuffer(text, np.uint8) if text else np.zeros(1, np.uint8), len(text), False, expected, fmt, None, 0)[0] == code


def test_capacity_protocol(ctx):
    import torch

    text = bc.random_netlist(300, 11, mand_every=7)
    _, want, recs, info = bc.host_parse(text, [1, 0], 0)
    src = np.frombuffer(text, np.uint8)
    rc, n, got = bc.device_parse(ctx, src, len(text), False, [1, 0], 0, None, 0)
    assert (rc, n, got) == (bc.ARG, want, info)
    canary = torch.full((want + 3, REC), 0x5A, dtype=torch.uint8, device="cuda")
    rc, n, got = bc.device_parse(ctx, src, len(text), False, [1, 0], 0, canary, want - 1)
    torch.cuda.synchronize()
    assert (rc, n, got) == (bc.ARG, want, info)
    assert bool((canary == 0x5A).all()), "a call that reports the capacity wrote records"
    rc, n, got = bc.device_parse(ctx, src, len(text), False, [1, 0], 0, canary, want)
    torch.cuda.synchronize()
    assert (rc, n, got) == (0, want, info)
    assert canary[:want].cpu().numpy().tobytes() == recs and bool((canary[want:] == 0x5A).all())


def test_argument_checks(ctx):
    import torch

    text = np.frombuffer(bc.random_netlist(5, 1), np.uint8)
    host_ops = torch.zeros((64, REC), dtype=torch.uint8)
    d_ops = torch.zeros((64 * REC + 8,), dtype=torch.uint8, device="cuda")
    assert bc.device_parse(ctx, text, text.size, False, None, 0, host_ops, 64)[0] == bc.ARG  # d_ops in host memory
    assert bc.device_parse(ctx, text, text.size, False, None, 0, d_ops[1:], 64)[0] == bc.ARG  # not 8-byte aligned
    assert bc.device_parse(ctx, text, text.size, False, None, 0, d_ops, 1 << 40)[0] == bc.ARG  # beyond its allocation
    assert bc.device_parse(ctx, text, text.size, True, None, 0, d_ops, 64)[0] == bc.ARG  # "device" text in host memory
    t, addr = on_gpu(text.tobytes())
    assert bc.device_parse(ctx, addr, 1 << 40, True, None, 0, d_ops, 64)[0] == bc.ARG  # text beyond its allocation
    assert bc.device_parse(ctx, addr, text.size, True, None, 0, d_ops, 64)[0] == 0


@pytest.mark.parametrize("tail", [b"2 1 0 1 2 XOR\n2 1 0 1 3 AND\n", b"7", b"\n2 1 0 1 2 XOR\n"], ids=["more-gate-lines", "a-digit", "a-line-after-lf"])
@pytest.mark.parametrize("final_newline", [True, False])
def test_reads_stay_inside_len(ctx, tail, final_newline):
    """the bytes right behind the text read as more of it -- further gate lines, a digit that would extend the last number (a kind,
    with a final number only in a text that breaks off): the answer is that of the text alone (no guard page, no fault: the bytes
    behind lie in the same allocation)"""
    import torch

    tile, _ = bc.tiles()
    for text in (bc.fashion(4, 1, 8, [b"2 1 0 1 4 XOR", b"2 1 0 4 5 AND", b"1 1 5 6 INV"]), bc.of_length(tile, 3), bc.of_length(2 * tile + 5, 4)):
        if not final_newline:
            text = text[:-1]
        cut = text[:-4]  # breaks off inside the last line: "... 1 1 5 6" -- the digit behind would make it "67"
        for t in (text, cut):
            rc, n, recs, info = bc.host_parse(t, None, 0)
            keep, addr = on_gpu(t, lead=5, tail=tail)
            d_ops = torch.zeros((n + 8, REC), dtype=torch.uint8, device="cuda")
            got = bc.device_parse(ctx, addr, len(t), True, None, 0, d_ops, n + 8)
            torch.cuda.synchronize()
            assert got[0] == rc and got[1] == n
            if rc == 0:
                assert got[2] == info and d_ops[:n].cpu().numpy().tobytes() == recs


def test_header_claiming_all_memory(ctx):
    """2^32 - 1 inputs in a few bytes: the sizing call reports the count and allocates nothing of that size"""
    import torch

    text = b"1 4294967295\n1 4294967295\n1 1\n2 1 0 1 4294967294 XOR\n"
    src = np.frombuffer(text, np.uint8)
    bc.device_parse(ctx, src, len(text), False, None, 0, None, 0)  # (the arena's first blocks)
    free0 = torch.cuda.mem_get_info()[0]
    t0 = time.perf_counter()
    rc, n, info = bc.device_parse(ctx, src, len(text), False, None, 0, None, 0)
    dt = time.perf_counter() - t0
    assert (rc, n) == (bc.ARG, 1 << 32)  # the inputs and the one gate
    assert info["n_inputs"] == (1 << 32) - 1 and info["n_xor"] == 1
    assert free0 - torch.cuda.mem_get_info()[0] < (64 << 20) and dt < 0.5
    small = torch.zeros((16, REC), dtype=torch.uint8, device="cuda")
    assert bc.device_parse(ctx, src, len(text), False, None, 0, small, 16)[:2] == (bc.ARG, 1 << 32)


def test_end_to_end_proof(rv, ctx, big_texts, rule_seeds):
    from reverie_amd import bristol

    text = big_texts[0][1]
    a, b = 0x0123456789ABCDEF, 0xFEDCBA9876543210
    wit = [(a >> i) & 1 for i in range(64)] + [(b >> i) & 1 for i in range(64)]
    exp = [(((a + b) & (2**64 - 1)) >> i) & 1 for i in range(64)]
    prog, info = bristol.parse(text, expected_outputs=exp)
    want = bytes(rv.Proof.new(rv.Circuit(prog, info["wire_counts"]), wit, [], seeds=rule_seeds))
    for src in (text, memoryview(text), np.frombuffer(text, np.uint8), on_gpu(text, lead=0, tail=b"")[0][:len(text)]):
        ops, dinfo = bristol.parse_device(src, expected_outputs=exp)
        assert dinfo == info and tuple(ops.shape) == (len(prog), REC)
        assert ops.cpu().numpy().tobytes() == prog.tobytes()
        circuit = rv.Circuit.from_device_ops(ops, dinfo["wire_counts"])
        proof = rv.Proof.new(circuit, wit, [], seeds=rule_seeds)
        assert bytes(proof) == want
        assert proof.verify(circuit)
    small, sinfo = bristol.parse(text, expected_outputs=exp, compact=True)
    dsmall, dsinfo = bristol.parse_device(text, expected_outputs=exp, compact=True)
    assert dsmall.cpu().numpy().tobytes() == small.tobytes() and dsinfo == sinfo
    # a zero-gate text and a MAND text go through the sizing call of the wrapper
    for t in (b"0 4\n1 4\n1 2\n", bc.long_mand(65)):
        p, i = bristol.parse(t)
        d, di = bristol.parse_device(t)
        assert d.cpu().numpy().tobytes() == p.tobytes() and di == i
    with pytest.raises(rv.ReverieError) as e:
        bristol.parse_device(bc.error_texts()[0][1])
    assert e.value.code == bc.error_texts()[0][4]
