"""rv_program_from_bincode_device against rv_program_from_bincode (the definition): the same records byte for byte, the same count,
info and return code for every file of the shared corpus (bincode_cases.py), from host bytes and from bytes in GPU memory at every
alignment; reads that stay inside `len`; the capacity protocol; rv_program_to_bincode_device against rv_program_to_bincode;
device-read programs through compile and proof, and through the command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bincode_cases as bc
from conftest import GOLDEN, ROOT, golden_ops
from reverie_amd.ops import OP_DTYPE, program

pytestmark = pytest.mark.gpu
REC = OP_DTYPE.itemsize


@pytest.fixture(scope="module")
def rv():
    import reverie_amd

    return reverie_amd


@pytest.fixture(scope="module")
def ctx(rv):
    return rv.Context.default()


def on_gpu(data: bytes, lead=0, tail=b"\x00\x00\x00\x00\x02\x00\x00\x00" * 6):
    """(tensor, device address of the data): the data `lead` bytes into a GPU allocation, `tail` (that reads as more records) behind it"""
    import torch

    t = torch.from_numpy(np.frombuffer(b"\xee" * lead + data + tail, np.uint8).copy()).cuda()
    return t, t.data_ptr() + lead


def check(ctx, data: bytes):
    """the device reader's answer for `data` in host memory and in GPU memory at leads 0 .. 3 is the host reader's"""
    import torch

    rc, n, recs = bc.host_parse(data)
    want_info = bc.expected_info(data, recs) if rc == 0 else None
    count = bc.count_of(data) if len(data) >= 8 else 0
    cap = (count if count <= len(data) // 16 else 0) + 2
    sources = [(np.frombuffer(data, np.uint8) if data else np.zeros(1, np.uint8), False, None)]
    for lead in range(4):
        keep, addr = on_gpu(data, lead)
        sources.append((addr, True, keep))
    for src, on_dev, keep in sources:
        d_ops = torch.full((cap, REC), 0xA5, dtype=torch.uint8, device="cuda")
        got_rc, got_n, got_info = bc.device_parse(ctx, src, len(data), on_dev, d_ops, cap)
        torch.cuda.synchronize()
        assert got_rc == rc, (got_rc, rc, on_dev)
        assert got_n == n
        if rc == 0:
            out = d_ops.cpu().numpy().tobytes()
            assert out[:n * REC] == recs
            assert out[n * REC:] == b"\xA5" * ((cap - n) * REC), "records beyond n_ops were written"
            assert got_info == want_info
    # a sizing call answers with the bytes' own code, or RV_E_ARG and the count
    got_rc, got_n, got_info = bc.device_parse(ctx, sources[0][0], len(data), False, None, 0)
    if rc or n == 0:
        assert (got_rc, got_n) == (rc, 0)
    else:
        assert (got_rc, got_n, got_info) == (bc.ARG, n, want_info)
    return rc, n, recs


def test_every_record_kind(ctx):
    prog = bc.every_kind()
    rc, n, recs = check(ctx, bc.program_file.dumps(prog))
    assert rc == 0 and recs == prog.tobytes()
    assert check(ctx, bc.program_file.dumps(program([])))[:2] == (0, 0)
    assert check(ctx, bc.program_file.dumps(prog[37:38]))[:2] == (0, 1)


def test_every_entry_offset(ctx):
    T, _ = bc.tiles()
    entries = set()
    for e in range(32):
        data = bc.entry_offset_case(e)
        starts, end = bc.record_starts(data)
        assert end == len(data)
        entries.add(min(s for s in starts if s >= T) % T)  # (tiles are counted from data[0]: the hook's comment)
        assert check(ctx, data)[0] == 0
    assert entries == set(range(32)), "the 32 cases must enter tile 1 at 32 distinct offsets"


@pytest.mark.parametrize("name,data", bc.boundary_cases(), ids=[c[0] for c in bc.boundary_cases()])
def test_around_tiles_and_scan_block(ctx, name, data):
    rc, n, _ = check(ctx, data)
    assert rc == (bc.BAD_OP if name.endswith("count+1") else 0)


def test_error_parity_single_defects(ctx):
    for name, data, code in bc.single_defect_cases():
        assert check(ctx, data)[0] == code, name


def test_error_parity_truncations(ctx):
    for name, data in bc.truncation_cases():
        assert check(ctx, data)[0] == bc.BAD_OP, name


@pytest.mark.parametrize("name,data,code", bc.ordering_cases(), ids=[c[0] for c in bc.ordering_cases()])
def test_error_ordering(ctx, name, data, code):
    assert check(ctx, data)[0] == code


def test_headers(ctx):
    import torch

    for name, data in bc.header_cases():
        assert check(ctx, data)[0] == bc.BAD_OP, name
    # a count no file of this length can hold: answered from the header, nothing of the count's size is asked of the arena
    data = bc.with_count(bc.program_file.dumps(bc.every_kind()), (1 << 64) - 1)
    src = np.frombuffer(data, np.uint8)
    bc.device_parse(ctx, src, len(data), False, None, 0)  # (the arena's first blocks)
    free0 = torch.cuda.mem_get_info()[0]
    assert bc.device_parse(ctx, src, len(data), False, None, 0)[:2] == (bc.BAD_OP, 0)
    assert free0 - torch.cuda.mem_get_info()[0] < (64 << 20)


def test_reads_stay_inside_len(ctx):
    """the data at the very end of a GPU tensor's storage; A: len cuts a record the full tensor would hold, B: len ends on a record and
    more valid records follow.  The answers are the host reader's for exactly len bytes."""
    import torch

    T, _ = bc.tiles()
    for total in (T + 5, 2 * T, 701):
        whole = bc.mix_of_length(total, 300 + total)
        starts, _ = bc.record_starts(whole)
        n = len(starts)
        for cut, count in ((starts[n // 2] + 9, n // 2 + 1), (starts[-1] + 3, n), (starts[n // 2], n // 2), (starts[-1], n - 1), (len(whole), n)):
            data = bc.with_count(whole[:cut], count)
            rc, want_n, recs = bc.host_parse(data)
            t = torch.from_numpy(np.frombuffer(bc.with_count(whole, count), np.uint8).copy()).cuda()  # the full file behind len
            end = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()  # ... and nothing behind it
            for keep, addr in ((t, t.data_ptr()), (end, end.data_ptr())):
                d_ops = torch.zeros((n + 1, REC), dtype=torch.uint8, device="cuda")
                got = bc.device_parse(ctx, addr, len(data), True, d_ops, n + 1)
                torch.cuda.synchronize()
                assert got[:2] == (rc, want_n), (total, cut, count)
                if rc == 0:
                    assert d_ops[:want_n].cpu().numpy().tobytes() == recs and got[2] == bc.expected_info(data, recs)


def test_capacity_and_arguments(ctx):
    import torch

    data = bc.mix_of_length(3000, 41)
    rc, want, recs = bc.host_parse(data)
    info = bc.expected_info(data, recs)
    src = np.frombuffer(data, np.uint8)
    assert bc.device_parse(ctx, src, len(data), False, None, 0) == (bc.ARG, want, info)
    canary = torch.full((want + 3, REC), 0x5A, dtype=torch.uint8, device="cuda")
    assert bc.device_parse(ctx, src, len(data), False, canary, want - 1) == (bc.ARG, want, info)
    torch.cuda.synchronize()
    assert bool((canary == 0x5A).all()), "a call that reports the capacity wrote records"
    assert bc.device_parse(ctx, src, len(data), False, canary, want) == (0, want, info)
    torch.cuda.synchronize()
    assert canary[:want].cpu().numpy().tobytes() == recs and bool((canary[want:] == 0x5A).all())
    assert bc.device_parse(ctx, src, len(data), False, canary, want, null_info=True)[:2] == (0, want)
    flat = torch.zeros(((want + 1) * REC + 8,), dtype=torch.uint8, device="cuda")
    assert bc.device_parse(ctx, src, len(data), False, flat.data_ptr() + 1, want)[0] == bc.ARG  # a misaligned d_ops
    assert bc.device_parse(ctx, src, len(data), False, torch.zeros((want, REC), dtype=torch.uint8), want)[0] == bc.ARG  # d_ops in host memory
    assert bc.device_parse(ctx, src, len(data), False, flat, 1 << 40)[0] == bc.ARG  # beyond its allocation
    assert bc.device_parse(ctx, src, len(data), False, canary, want, null_n=True)[0] == bc.ARG  # a null n_ops
    assert bc.device_parse(ctx, src, len(data), True, canary, want)[0] == bc.ARG  # a host pointer passed as device data
    keep, addr = on_gpu(data, 1)
    assert bc.device_parse(ctx, addr, 1 << 40, True, canary, want)[0] == bc.ARG  # data beyond its allocation
    assert bc.device_parse(ctx, addr, len(data), True, canary, want)[:2] == (0, want)


def writer_programs():
    out = [("every-kind", bc.every_kind().tobytes()), ("empty", b""), ("one", bc.every_kind()[5:6].tobytes())]
    for name, data in bc.boundary_cases():
        if not name.endswith(("garbage", "count+1")):
            out.append((name, bc.host_parse(data)[2]))
    return out


def test_writer(rv, ctx):
    import torch

    from reverie_amd import program_file

    for name, recs in writer_programs():
        rc, want = bc.host_write(recs)
        assert rc == 0
        for lead in (0, 8):  # (the records 8-byte aligned, on and off a 16-byte boundary)
            store = torch.from_numpy(np.frombuffer(b"\0" * lead + recs + b"\0" * 8, np.uint8).copy()).cuda()
            ops = store[lead:lead + len(recs)].view(-1, REC)
            got = program_file.dumps_device(ops)
            assert got.cpu().numpy().tobytes() == want, name
        # ... and back: the device reader on the device writer's bytes
        back, info = program_file.loads_device(got)
        assert back.cpu().numpy().tobytes() == program_file.loads(want).tobytes() == recs
        assert info == {**bc.expected_info(want, recs), "wire_counts": info["wire_counts"]} and info["wire_counts"] == (info["z64_wires"], info["gf2_wires"])
    # the output at every alignment, with a sentinel around it
    recs = writer_programs()[3][1]
    _, want = bc.host_write(recs)
    ops = torch.from_numpy(np.frombuffer(recs, np.uint8).copy()).cuda()
    n = len(recs) // REC
    for lead in range(17):
        out = torch.full((lead + len(want) + 33,), 0x5A, dtype=torch.uint8, device="cuda")
        assert bc.device_write(ctx, ops, n, out[lead:], len(want)) == (0, len(want))
        torch.cuda.synchronize()
        got = out.cpu().numpy().tobytes()
        assert got == b"\x5A" * lead + want + b"\x5A" * 33, lead
    # the capacity protocol
    assert bc.device_write(ctx, ops, n, None, 0) == (bc.ARG, len(want))
    out = torch.full((len(want),), 0x5A, dtype=torch.uint8, device="cuda")
    assert bc.device_write(ctx, ops, n, out, len(want) - 1) == (bc.ARG, len(want))
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all()), "a call that reports the size wrote bytes"
    # bad records, first / middle / last: the host writer's code
    base = np.frombuffer(recs, OP_DTYPE)
    for field, value in (("reserved", 1), ("domain", 4), ("opcode", 10)):
        for i in (0, n // 2, n - 1):
            prog = base.copy()
            if field == "opcode":
                prog["domain"][i] = 1
            prog[field][i] = value
            assert bc.host_write(prog.tobytes())[0] == bc.BAD_OP
            d = torch.from_numpy(prog.view(np.uint8).copy()).cuda()
            assert bc.device_write(ctx, d, n, out, len(want)) == (bc.BAD_OP, 0), (field, i)
            assert bc.device_write(ctx, d, n, None, 0) == (bc.BAD_OP, 0)
    # GF(2) immediates are written as imm & 1
    prog = program([bc.GF2.Const(1, 3), bc.GF2.AddConst(1, 2, 2)])
    assert program_file.dumps_device(torch.from_numpy(prog.view(np.uint8).copy()).cuda().view(-1, REC)).cpu().numpy().tobytes() == program_file.dumps(prog)


META = json.load(open(os.path.join(GOLDEN, "proofs.json")))


@pytest.mark.parametrize("name", ["adder64", "z64_mix"])
def test_end_to_end_proof(rv, rule_seeds, name):
    from reverie_amd import program_file
    from reverie_amd.ops import largest_wires

    m = META[name]
    prog = program(golden_ops(m))
    w2, w64 = m["wit_gf2"], [int(x) for x in m["wit_z64"]]
    data = program_file.dumps(prog)
    host_prog = program_file.loads(data)
    wc = tuple(int(x) for x in largest_wires(host_prog))  # (what the command line takes for a host-parsed program file)
    assert host_prog.tobytes() == prog.tobytes() and wc[0] <= m["wire_counts"][0] and wc[1] <= m["wire_counts"][1]
    want = bytes(rv.Proof.new(rv.Circuit(host_prog, wc), w2, w64, seeds=rule_seeds))
    for src in (data, np.frombuffer(data, np.uint8), on_gpu(data, 0, b"")[0]):
        ops, info = program_file.loads_device(src)
        assert ops.cpu().numpy().tobytes() == host_prog.tobytes() and info["wire_counts"] == wc
        circuit = rv.Circuit.from_device_ops(ops, info["wire_counts"], device_z64=True)
        proof = rv.Proof.new(circuit, w2, w64, seeds=rule_seeds)
        assert bytes(proof) == want
        assert proof.verify(circuit)
        assert proof.verify(rv.Circuit(host_prog, wc))


CLI_CHILD = """
import sys
import numpy as np
from reverie_amd.__main__ import main
from reverie_amd.proof import Proof
seeds = np.load(sys.argv[1])
plain_new = Proof.new
Proof.new = staticmethod(lambda circuit, wit_gf2, wit_z64, *a, **k: plain_new(circuit, wit_gf2, wit_z64, *a, **{**k, "seeds": seeds}))
sys.exit(main(sys.argv[2:]))
"""


def test_cli_in_a_child_process(tmp_path, rule_seeds):
    """`--program-format mcircuit-bincode --parser device` writes the proof file `--parser host` writes (the command line draws its
    seeds from the OS: the child puts fixed ones in their place)"""
    from reverie_amd import program_file

    m = META["adder64"]
    (tmp_path / "adder.bin").write_bytes(program_file.dumps(program(golden_ops(m))))
    (tmp_path / "wit.txt").write_text(" ".join(str(b) for b in m["wit_gf2"]))
    np.save(tmp_path / "seeds.npy", rule_seeds)
    (tmp_path / "child.py").write_text(CLI_CHILD)
    env = {**os.environ, "PYTHONPATH": ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")}

    def run(*args):
        common = ["--program-path", str(tmp_path / "adder.bin"), "--program-format", "mcircuit-bincode"]
        return subprocess.run([sys.executable, str(tmp_path / "child.py"), str(tmp_path / "seeds.npy")] + list(args) + common, env=env,
                              capture_output=True, text=True, timeout=300)

    proofs = []
    for k, extra in enumerate((["--parser", "host"], ["--parser", "device"], ["--parser", "device", "--compiler", "device"])):
        path = tmp_path / f"proof{k}.bin"
        r = run("--operation", "prove", "--witness-path", str(tmp_path / "wit.txt"), "--proof-path", str(path), *extra)
        assert r.returncode == 0, r.stderr[-2000:]
        proofs.append(path.read_bytes())
    assert proofs[0] == proofs[1] == proofs[2] and len(proofs[0]) > 1000
    r = run("--operation", "verify", "--proof-path", str(tmp_path / "proof0.bin"), "--parser", "device")
    assert r.returncode == 0 and "Ok(())" in r.stdout, r.stderr[-2000:]
    r = run("--operation", "oneshot", "--witness-path", str(tmp_path / "wit.txt"), "--parser", "device", "--evaluator", "host")
    assert r.returncode != 0 and "--evaluator host" in r.stderr
