"""tests/fs_ref.py and tests/fs_cases.py against the CPU oracle, the committed known answers and a golden proof (no GPU): the reference
the Fiat-Shamir and record-head kernels are compared with (tests/test_gpu_open_heads.py) is tied down here first."""
import json
import os

import numpy as np
import pytest

import fs_cases
import fs_ref
import proof_mutate
from conftest import GOLDEN
from test_oracle_golden import load_case

PRIMITIVES = json.load(open(os.path.join(GOLDEN, "primitives.json")))


def test_opening_known_answers(oracle):
    assert len(PRIMITIVES["challenge"]) >= 2
    for e in PRIMITIVES["challenge"]:
        c = np.frombuffer(bytes.fromhex(e["comm"]), np.uint8)
        omit, done_at, drawn = fs_ref.opening(c)
        assert omit.tolist() == e["omit"] == oracle.challenge(c).tolist()
        assert (omit < 8).sum() == 40 and 39 <= done_at < len(drawn)


def test_opening_equals_oracle_on_random_commitments(oracle):
    rng = np.random.default_rng(2000)
    for i in range(2000):
        c = rng.integers(0, 256, 32, dtype=np.uint8)
        omit, done_at, drawn = fs_ref.opening(c)
        assert np.array_equal(omit, oracle.challenge(c)), f"commitment {i}: {c.tobytes().hex()}"
        # the replay's own bookkeeping: the draw that reached 40 is a first draw of its repetition, and 39 stood before it
        assert len({int(r) for r in drawn[:done_at, 0]}) == 39 and int(drawn[done_at, 0]) not in {int(r) for r in drawn[:done_at, 0]}


@pytest.mark.parametrize("name", ["gf2_mix", "z64_mix"])
def test_comm_equals_oracle_commit(oracle, rule_seeds, name):
    m, prog, w2, w64, wc, gold = load_case(name)
    h, _, comm = oracle.commit(prog, w2, w64, wc, rule_seeds, threads=4)
    assert fs_ref.comm(h).tobytes() == comm.tobytes() == gold[:32]
    assert fs_ref.opening(fs_ref.comm(h))[0].tolist() == m["omit"]


@pytest.mark.parametrize("name", ["gf2_mix", "z64_mix"])
def test_layout_and_heads_reserialise_golden_proof(name):
    """layout + heads + frame, filled with the vectors cut out of the golden proof, give the proof back byte for byte"""
    gold = open(os.path.join(GOLDEN, f"proof_{name}.bin"), "rb").read()
    comm, domains = proof_mutate.parse(gold)
    omit = fs_ref.opening(np.frombuffer(comm, np.uint8))[0]
    on = [int(r) for r in np.nonzero(omit < 8)[0]]
    off = [int(r) for r in np.nonzero(omit == 8)[0]]
    assert [rec[0] for rec in domains[0][0]] == [int(omit[r]) for r in on] == [rec[0] for rec in domains[1][0]]
    lens = [len(v) for d in (0, 1) for v in domains[d][0][0][2]]
    # the inputs of heads(): what the proof holds, and noise where the proof holds nothing (the omitted player's key, the opened
    # repetitions' seeds and digests, the others' keys)
    rng = np.random.default_rng(7)
    seeds = rng.integers(0, 256, (256, 16), dtype=np.uint8)
    keys = rng.integers(1, 256, (256, 128), dtype=np.uint8)
    h_on = [rng.integers(0, 256, (256, 32), dtype=np.uint8) for _ in (0, 1)]
    for j, r in enumerate(on):
        k = np.frombuffer(domains[0][0][j][1], np.uint8).copy()
        assert domains[1][0][j][1] == domains[0][0][j][1] and not k[16 * omit[r]:16 * omit[r] + 16].any()
        k[16 * omit[r]:16 * omit[r] + 16] = keys[r, 16 * omit[r]:16 * omit[r] + 16]
        keys[r] = k
    for j, r in enumerate(off):
        for d in (0, 1):
            pre = domains[d][1][48 * j:48 * j + 48]
            if d == 0:
                seeds[r] = np.frombuffer(pre[:16], np.uint8)
            assert pre[:16] == seeds[r].tobytes()
            h_on[d][r] = np.frombuffer(pre[16:], np.uint8)
    table, ol, (n_on, n_pre), end = fs_ref.layout(omit, lens, 0, True)
    assert (n_on, n_pre, end) == (40, 216, len(gold)) and ol["rep"] == on and ol["n"] == 40
    pieces = dict(fs_ref.frame(comm, n_on, n_pre, lens))
    pieces.update(fs_ref.heads(omit, seeds, keys, h_on[0].view("<u4"), h_on[1], table, lens))  # (digests as words and as bytes)
    for j, r in enumerate(on):
        for d in (0, 1):
            for v in range(3):
                if domains[d][0][j][2][v]:  # (an empty vector starts where the next length field does)
                    pieces[int(table[2 + 3 * d + v, r])] = domains[d][0][j][2][v]
        assert ol["dst"][j] == int(table[3, r])
    img = fs_ref.image(0xA5, end, pieces)
    assert sum(len(b) for b in pieces.values()) == end  # every byte of the proof is some piece's: nothing overlaps, nothing is left
    assert img.tobytes() == gold


def test_layout_unframed_sections_follow_the_counts():
    """a shard's sections lie one behind the other from base0, sized by its own numbers of opened and unopened repetitions"""
    omit = fs_cases.case("crowded32")[2]
    rb, R = fs_cases.own_shard("crowded32", omit)
    lens = (3, 130, 2, 8, 16, 24)
    table, ol, (n_on, n_pre), end = fs_ref.layout(omit[rb:rb + R], lens, 5, False)
    sz2, sz64 = fs_ref.record_sizes(lens)
    assert (sz2, sz64) == (153 + 135, 153 + 48) and n_on >= 13 and n_on + n_pre == R
    assert end == 5 + n_on * (sz2 + sz64) + 2 * 48 * n_pre
    on = np.nonzero(omit[rb:rb + R] < 8)[0]
    assert table[0, on[0]] == 5 and table[1, on[0]] == 5 + n_on * sz2 + 48 * n_pre and (table[2:, omit[rb:rb + R] == 8] == 0).all()
    assert ol["rep"] == on.tolist()


def test_mailbox_words():
    d, comm, omit, _, _ = fs_cases.case("plain")
    w = fs_ref.mailbox(comm, omit, 3, 29)
    assert w.shape == (74,) and w[:8].astype("<u4").tobytes() == comm.tobytes() and w[8:72].astype("<u4").tobytes() == omit.tobytes() and w[72:].tolist() == [3, 29]


@pytest.mark.parametrize("name", fs_cases.NAMES)
def test_named_set_has_its_property(name):
    d, comm, omit, done_at, drawn = fs_cases.case(name)
    assert (omit < 8).sum() == 40
    assert fs_cases.holds(name, omit, done_at, drawn), name
    own = fs_cases.own_shard(name, omit)
    if name.startswith("empty"):
        assert (omit[own[0]:own[0] + own[1]] == 8).all()
    if name == "crowded32":
        assert (omit[own[0]:own[0] + 32] < 8).sum() >= 13
    if name == "crowded64":
        assert (omit[own[0]:own[0] + 64] < 8).sum() >= 20
    if name in ("redraw", "late"):
        # the property changes the answer: a replay that keeps the first player / one that goes on to draw 128 gives another map
        first, to_end = np.full(256, 8, np.uint8), omit.copy()
        for rep, player in drawn[:done_at + 1]:
            if first[rep] == 8:
                first[rep] = player
        for rep, player in drawn[done_at + 1:128]:
            if to_end[rep] < 8:
                to_end[rep] = player
        assert not np.array_equal(first if name == "redraw" else to_end, omit)


def test_named_sets_are_distinct():
    comms = {fs_cases.case(n)[1].tobytes() for n in fs_cases.NAMES}
    assert len(comms) == len(fs_cases.NAMES)
