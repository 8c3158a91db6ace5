"""Witness texts at the edges of the device parser's tiles (shared by test_witness_text_host.py and test_gpu_witness_text.py), the
writer's line lengths, and the three-line model of the writer.  T is the tile size rv_hook_witness_text_tiles reports."""
import numpy as np

ARG, UNSUPPORTED, WITNESS_SHORT = 9, 8, 2
NEAR_MISSES = bytes([ord("/"), ord("2"), 0xB0, 0xB1, 0x00])


def lengths(T):
    return [0, 1, 15, 16, 17, T - 1, T, T + 1, 2 * T - 1, 2 * T + 1, 5 * T + 3]


def _content(kind, n, rng):
    if kind == "kept":
        return (rng.integers(0, 2, n, dtype=np.uint8) + 0x30).tobytes()
    if kind == "none":
        return bytes(NEAR_MISSES[i % len(NEAR_MISSES)] for i in range(n))
    if kind == "alternating":
        a = np.frombuffer(bytes(NEAR_MISSES[i % len(NEAR_MISSES)] for i in range(n)), np.uint8).copy()
        a[::2] = rng.integers(0, 2, len(a[::2]), dtype=np.uint8) + 0x30
        return a.tobytes()
    if kind == "random":
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    if kind == "crlf":  # lines of 62 bits and CR LF
        a = rng.integers(0, 2, n, dtype=np.uint8) + 0x30
        a[62::64] = 13
        a[63::64] = 10
        return a.tobytes()
    if kind == "near":  # mostly bits, a near miss every third byte
        a = rng.integers(0, 2, n, dtype=np.uint8) + 0x30
        a[1::3] = np.frombuffer(bytes(NEAR_MISSES[i % len(NEAR_MISSES)] for i in range(len(a[1::3]))), np.uint8)
        return a.tobytes()
    raise ValueError(kind)


KINDS = ("kept", "none", "alternating", "random", "crlf", "near")


def texts(T):
    """[(name, bytes)]: every content kind at every length, a lone kept byte at each of the first and last three positions of a
    tile, and a run of kept bytes that ends exactly at a tile edge, followed by a tile with none"""
    rng = np.random.default_rng(20261021)
    out = [(f"{kind}-{n}", _content(kind, n, rng)) for kind in KINDS for n in lengths(T)]
    for tile in (0, 1):
        for pos in (0, 1, 2, T - 3, T - 2, T - 1):
            a = bytearray(b"\n" * (2 * T + 5))
            a[tile * T + pos] = ord("1")
            out.append((f"lone-{tile}-{pos}", bytes(a)))
    out.append(("run-to-edge", b"x" * 100 + _content("kept", T - 100, rng) + b" " * T + b"01"))
    out.append(("run-to-edge-2", _content("kept", 2 * T, rng) + b"\r\n" * (T // 2) + b"1"))
    return out


def short_texts(T):
    """the texts of at most 40 bytes (every two-way cut of them is tried), and a few more of those lengths"""
    rng = np.random.default_rng(7)
    extra = [(f"short-{kind}-{n}", _content(kind, n, rng)) for kind in ("alternating", "random", "near") for n in (2, 33, 40)]
    return [(n, t) for n, t in texts(T) if len(t) <= 40] + extra


def edge_texts(T):
    """the texts that reach a tile's edge (seeded random cuts of them are tried)"""
    return [(n, t) for n, t in texts(T) if len(t) >= T - 1]


def line_bits_values(n):
    return [0, 1, 7, 16, 64, n, n + 1]


def write_model(bits, line_bits):
    """rv_witness_write, said in three lines"""
    n = len(bits)
    ends = [i for i in range(n) if (line_bits and (i + 1) % line_bits == 0) or i == n - 1]
    return b"".join(bytes(48 + int(b) for b in bits[a:e + 1]) + b"\n" for a, e in zip([0] + [e + 1 for e in ends[:-1]], ends))


def fnv(data: bytes) -> int:
    h = 0xCBF29CE484222325
    for b in data:
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h
