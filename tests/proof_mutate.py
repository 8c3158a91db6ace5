"""Well-formed proofs with altered vector lengths -- TEST INFRASTRUCTURE (no GPU, no library import).

A proof is bincode 1.3 (fixint: u64 little-endian lengths) of

    comm[32] | domain gf2 | domain z64
    domain = u64 n_online | n_online x record | u64 n_pre | n_pre x (seed[16] | comm_online[32])
    record = omit[1] | keys[128] | u64 len, rec | u64 len, corr | u64 len, in

`parse` takes it apart, `serialise` puts it together again (bit-exact round trip), and `catalogue` yields mutated proofs in which
lengths and bytes move TOGETHER: every entry parses, so it reaches the verifier's own length rules (the group's first record
decides the length, short vectors read as zero, extra bytes are ignored) instead of dying in the parser as a proof with one
overwritten length field does."""
from __future__ import annotations

import hashlib
import struct

VECTORS = ("rec", "corr", "in")
DOMAINS = ("gf2", "z64")
GROUPS = (0, 4)  # the first and the last online group (records 8g .. 8g+7 of the 40 online records)
# (name, group or None): which records of a domain a change is applied to
ALL_TARGETS = tuple((t, g) for g in GROUPS for t in ("r0", "r3", "r7", "all8")) + (("all40", None),)
THIN_TARGETS = tuple((t, g) for g in GROUPS for t in ("r0", "r3", "all8"))  # (what slow entry points keep: see catalogue)


def parse(proof: bytes):
    """-> (comm, [gf2, z64]); a domain is (records, preprocessing_bytes), a record [omit, keys(128), [rec, corr, in]] (bytes).
    The proof must end where its second domain ends."""
    proof = bytes(proof)
    u64 = lambda at: struct.unpack_from("<Q", proof, at)[0]  # noqa: E731
    comm, pos, domains = proof[:32], 32, []
    if len(comm) != 32:
        raise ValueError("proof shorter than its commitment")

    def take(n):
        nonlocal pos
        if n > len(proof) - pos:
            raise ValueError(f"proof ends inside a field at byte {pos}")
        pos += n
        return proof[pos - n:pos]

    for _ in range(2):
        n = u64(pos)
        take(8)
        records = []
        for _ in range(n):
            omit = take(1)[0]
            keys = take(128)
            vecs = []
            for _ in range(3):
                ln = u64(pos)
                take(8)
                vecs.append(take(ln))
            records.append([omit, keys, vecs])
        n_pre = u64(pos)
        take(8)
        domains.append((records, take(48 * n_pre)))
    if pos != len(proof):
        raise ValueError(f"{len(proof) - pos} bytes behind the proof")
    return comm, domains


def serialise(comm: bytes, domains) -> bytes:
    out = [bytes(comm)]
    for records, pre in domains:
        out.append(struct.pack("<Q", len(records)))
        for omit, keys, vecs in records:
            out.append(bytes([omit]))
            out.append(bytes(keys))
            for v in vecs:
                out.append(struct.pack("<Q", len(v)))
                out.append(bytes(v))
        assert len(pre) % 48 == 0
        out.append(struct.pack("<Q", len(pre) // 48))
        out.append(bytes(pre))
    return b"".join(out)


def _copy(domains):
    return [([[o, k, list(v)] for o, k, v in records], pre) for records, pre in domains]


def target_records(target):
    """the indices, among a domain's 40 online records, that a target names"""
    name, g = target
    if name == "all40":
        return list(range(40))
    if name == "all8":
        return list(range(8 * g, 8 * g + 8))
    return [8 * g + int(name[1:])]


def _target_label(target):
    return target[0] if target[1] is None else f"g{target[1]}.{target[0]}"


def split_label(label: str):
    """a catalogue label -> (domains, field, group or None, target, change); ("", "trailing", None, "", change) for the
    entries with bytes behind the proof"""
    head, change = label.split(":")
    if head == "trailing":
        return "", "trailing", None, "", change
    parts = head.split(".")
    group = int(parts[2][1:]) if len(parts) == 4 else None
    return parts[0], parts[1], group, parts[-1], change


def gf2_length_changes(n: int):
    """[(label, new length, fill byte or None)] for a GF(2) vector of n bytes: every change that is no change is left out, and
    of two cuts to the same length the first is kept"""
    cuts = [("to0", 0), ("to1", 1), ("len-1", n - 1), ("len-2", n - 2), ("len-3", n - 3), ("len-4", n - 4)]  # the end mask's 4 alignments
    cuts += [(f"to{k}", k) for k in (63, 64, 65, 127, 128, 129)]  # around the 64-byte unpack tile
    out, seen = [], set()
    for label, m in cuts:
        if 0 <= m < n and m not in seen:
            seen.add(m)
            out.append((label, m, None))
    for add in (1, 3, 8, 64):
        for fill in (0x00, 0xFF):
            out.append((f"+{add}x{fill:02X}", n + add, fill))
    return out


def z64_length_changes(n: int):
    cuts = [("-8", n - 8), ("-16", n - 16), ("to0", 0), ("to8", 8), ("-1", n - 1), ("-7", n - 7), ("-9", n - 9)]
    out, seen = [], set()
    for label, m in cuts:
        if 0 <= m < n and m not in seen:
            seen.add(m)
            out.append((label, m, None))
    for add in (1, 7, 8, 9):
        for fill in (0x00, 0xFF):
            out.append((f"+{add}x{fill:02X}", n + add, fill))
    return out


def _resize(v: bytes, m: int, fill):
    return v[:m] if m <= len(v) else v + bytes([fill]) * (m - len(v))


def catalogue(proof: bytes, targets=ALL_TARGETS, gf2_items=None, domains=DOMAINS, vectors=VECTORS, same_length=True):
    """Yields (label, mutated proof bytes) for a good proof, deterministically; every entry parses.

    Length changes: domain x vector x target x change (gf2_length_changes / z64_length_changes of the target's first record; the
    kept bytes are a prefix of the honest ones, added bytes are 0x00 or 0xFF).  `targets` thins the TARGET axis only (ALL_TARGETS,
    THIN_TARGETS); the length changes are never thinned.
    Same-length changes: the padding bits of a GF(2) vector's last byte set (gf2_items = {"rec": n, "corr": n, "in": n} names
    the item counts, so that all 8 - n % 8 padding bits are set; without it the one bit that is padding for every n), the
    omitted player's zeroed key slot filled, `omit` replaced by another player, and bytes appended behind the proof.
    `domains` / `vectors` keep the length changes of those only, same_length=False leaves the same-length changes out (a reduced
    catalogue for a large proof).  Entries whose bytes equal the good proof's or an earlier entry's are left out."""
    proof = bytes(proof)
    comm, good = parse(proof)
    seen = {hashlib.blake2b(proof).digest()}

    def emit(label, domains, tail=b""):
        data = serialise(comm, domains) + tail
        h = hashlib.blake2b(data).digest()
        if h in seen:
            return None
        seen.add(h)
        return label, data

    for d, dom in enumerate(DOMAINS):
        for v, vec in enumerate(VECTORS):
            if dom not in domains or vec not in vectors:
                continue
            for target in targets:
                recs = target_records(target)
                n0 = len(good[d][0][recs[0]][2][v])
                for label, m, fill in (gf2_length_changes if d == 0 else z64_length_changes)(n0):
                    mut = _copy(good)
                    for r in recs:
                        old = mut[d][0][r][2][v]
                        mut[d][0][r][2][v] = _resize(old, max(len(old) + (m - n0), 0), fill)
                    e = emit(f"{dom}.{vec}.{_target_label(target)}:{label}", mut)
                    if e:
                        yield e
    if not same_length:
        return
    # ---- same length, still well-formed
    for v, vec in enumerate(VECTORS):
        n_items = (gf2_items or {}).get(vec)
        pad = 0x01 if n_items is None else (1 << (8 - n_items % 8)) - 1
        for target in targets:
            mut = _copy(good)
            for r in target_records(target):
                old = mut[0][0][r][2][v]
                if old:
                    mut[0][0][r][2][v] = old[:-1] + bytes([old[-1] | pad])
            e = emit(f"gf2.{vec}.{_target_label(target)}:padbits", mut)
            if e:
                yield e
    for d, dom in enumerate(DOMAINS):
        for target in targets:
            mut = _copy(good)
            for r in target_records(target):
                omit, keys, _ = mut[d][0][r]
                if omit < 8:
                    mut[d][0][r][1] = keys[:16 * omit] + bytes(range(0xA0, 0xB0)) + keys[16 * omit + 16:]
            e = emit(f"{dom}.keys.{_target_label(target)}:omitted-slot", mut)
            if e:
                yield e
    for doms in ((0,), (1,), (0, 1)):
        for target in targets:
            if target[0] in ("all8", "all40"):
                continue
            for step in (1, 5):
                mut = _copy(good)
                for d in doms:
                    for r in target_records(target):
                        mut[d][0][r][0] = (mut[d][0][r][0] + step) % 8
                e = emit(f"{'+'.join(DOMAINS[d] for d in doms)}.omit.{_target_label(target)}:+{step}mod8", mut)
                if e:
                    yield e
    for n in (1, 4096):
        for fill in (0x00, 0xFF):
            e = emit(f"trailing:+{n}x{fill:02X}", good, bytes([fill]) * n)
            if e:
                yield e
