"""tests/proof_mutate.py on the CPU: the round trip is bit-exact, every catalogue entry is a proof the oracle can answer, and
the oracle ALONE separates the catalogue of each circuit of tests/verify_length_cases.py into accepted, refused and malformed
proofs -- so that tests/test_gpu_verify_lengths.py cannot degenerate into one class."""
import glob
import os

import pytest

import proof_mutate
import verify_length_cases as cases
from conftest import GOLDEN

MALFORMED = ("err", 4)  # RVO_E_PROOF_MALFORMED


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "proof_*.bin"))), ids=os.path.basename)
def test_round_trip_golden(path):
    proof = open(path, "rb").read()
    comm, domains = proof_mutate.parse(proof)
    assert proof_mutate.serialise(comm, domains) == proof
    assert [len(d[0]) for d in domains] == [40, 40] and [len(d[1]) for d in domains] == [216 * 48] * 2


def test_parse_refuses_what_is_not_a_whole_proof():
    proof = open(os.path.join(GOLDEN, "proof_gf2_mix.bin"), "rb").read()
    for bad in (proof[:-1], proof + b"\0", proof[:20]):
        with pytest.raises(ValueError):
            proof_mutate.parse(bad)


@pytest.mark.parametrize("name", cases.NAMES)
def test_catalogue_classes_by_the_oracle(oracle, rule_seeds, name):
    cs = cases.case(oracle, rule_seeds, name)
    good, entries, ans = cs["good"], cs["entries"], cs["answers"]
    comm, domains = proof_mutate.parse(good)
    assert proof_mutate.serialise(comm, domains) == good
    assert cases.answer(oracle, cs["prog"], cs["wc"], good) == (True, True)
    # deterministic, labelled once, and every entry is a whole proof (plus, for the trailing entries, bytes behind it)
    again = list(proof_mutate.catalogue(good, gf2_items=cases.gf2_items(cs["prog"])))
    assert again == entries
    labels = [e[0] for e in entries]
    assert len(set(labels)) == len(labels) and len({e[1] for e in entries} | {good}) == len(entries) + 1
    for label, data in entries:
        if label.startswith("trailing:"):
            assert data.startswith(good) and len(data) > len(good)
        else:
            c2, d2 = proof_mutate.parse(data)
            assert proof_mutate.serialise(c2, d2) == data and c2 == comm, label
    # every answer is a bool or `malformed` (the oracle met nothing else, and did not crash)
    for (label, _), a in zip(entries, ans):
        for x in a:
            assert x is True or x is False or x == MALFORMED, (label, a)
        assert (a[0] == MALFORMED) == (a[1] == MALFORMED), (label, a)
    n_true, n_false, n_bad = cases.classes(ans)
    print(f"{name}: {len(entries)} entries: {n_true} accepted, {n_false} refused, {n_bad} malformed")
    assert min(n_true, n_false, n_bad) >= 10, f"{name}: {len(entries)} entries: {n_true} accepted, {n_false} refused, {n_bad} malformed"
    # the thinned target axis is a part of the whole one
    thin = {e[0] for e in proof_mutate.catalogue(good, targets=proof_mutate.THIN_TARGETS, gf2_items=cases.gf2_items(cs["prog"]))}
    assert thin and thin <= set(labels)


@pytest.mark.parametrize("name", ["MIX", "WIDE"])
def test_first_record_decides_the_length(oracle, rule_seeds, name):
    """gf2/recon.rs:241-259: `corr` and `in` are unpacked up to the FIRST record's length, the others only have to be as long.
    Record 0 shortened with records 1..7 honest is therefore a proof the reference answers (never malformed) -- with the same
    answer as all eight shortened, the longer records' bytes past record 0's end being ignored -- while a later record shortened
    alone is malformed.  `rec` must be equal in all eight (gf2/share.rs:157-164)."""
    cs = cases.case(oracle, rule_seeds, name)
    by = {e[0]: a for e, a in zip(cs["entries"], cs["answers"])}
    seen = 0
    for g in proof_mutate.GROUPS:
        for vec in ("corr", "in"):
            for change in ("to0", "to1", "len-1", "len-4", "to63", "to64", "to65"):
                first, all8, third = (by.get(f"gf2.{vec}.g{g}.{t}:{change}") for t in ("r0", "all8", "r3"))
                if first is None:
                    continue
                assert all8 is not None and third is not None
                assert first[0] != MALFORMED and first == all8, (vec, g, change, first, all8)
                assert third == (MALFORMED, MALFORMED), (vec, g, change, third)
                seen += 1
        for t in ("r0", "r3", "r7"):
            assert by[f"gf2.rec.g{g}.{t}:len-1"] == (MALFORMED, MALFORMED)
            assert by[f"gf2.rec.g{g}.{t}:+1x00"] == (MALFORMED, MALFORMED)
        assert by[f"gf2.rec.g{g}.all8:len-1"][0] != MALFORMED
        # a LONGER first record asks the others for bytes they do not have; longer later records are ignored
        assert by[f"gf2.corr.g{g}.r0:+8xFF"] == (MALFORMED, MALFORMED)
        assert by[f"gf2.corr.g{g}.r7:+8xFF"] == (True, True)
    assert seen >= 20


def test_z64_short_records_read_as_zero(oracle, rule_seeds):
    """z64/recon.rs:96-104, z64/share.rs:78-88: the item count is record 0's length / 8, shorter records read as zero item by
    item, a trailing partial word is dropped -- no Z64 length is malformed"""
    cs = cases.case(oracle, rule_seeds, "Z")
    by = {e[0]: a for e, a in zip(cs["entries"], cs["answers"])}
    z = {k: a for k, a in by.items() if k.startswith("z64.") and ".keys." not in k and ".omit." not in k}
    assert len(z) > 100 and all(a[0] != MALFORMED for a in z.values())
    for g in proof_mutate.GROUPS:
        for vec in proof_mutate.VECTORS:
            for t in ("r0", "r3", "r7", "all8"):
                for change in ("+1x00", "+7xFF", "+8xFF", "+9x00"):  # bytes past what the circuit consumes are ignored
                    assert z[f"z64.{vec}.g{g}.{t}:{change}"] == (True, True), (vec, g, t, change)
                assert z[f"z64.{vec}.g{g}.{t}:-7"] == z[f"z64.{vec}.g{g}.{t}:-8"] != (True, True)  # (a partial word is no item)
