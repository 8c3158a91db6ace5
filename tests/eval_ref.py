"""Independent batched reference of cleartext evaluation (rv_evaluate_batch), no GPU.

The semantics are those of `model()` in tests/test_gpu_eval.py (interpreter/single.rs, combine.rs), over a batch of witnesses:
GF(2) values are Python ints of B bits (bit b: witness b), Z64 values uint64[B] numpy arrays (wrapping mod 2^64), B2A the binary
number of its 64 source bits, a GF(2) witness byte counts as 1 when it is non-zero.

evaluate(prog, wc, w2, w64)        -> (gf2 [B][n2] uint8, z64 [B][n64] uint64, n_failed [B], first_failed_op [B], -1 for none)
evaluate_layers(prog, wc, w2, w64) -> the same, one layer of independent ops at a time (layered circuits: ~10^7 ops in seconds)
"""
import numpy as np

from reverie_amd.ops import (DOM_B2A, DOM_GF2, DOM_SIZEHINT, DOM_Z64, OP_ADD, OP_ADDCONST, OP_ASSERTZERO, OP_CONST, OP_INPUT, OP_MUL,
                             OP_MULCONST, OP_RANDOM, OP_SUB, OP_SUBCONST)

M64 = (1 << 64) - 1


def _witnesses(w2, w64):
    """([B][n2] bytes, [B][n64] words, B): either may be None (no columns); a 1-D witness is a batch of one"""
    if w2 is not None:
        w2 = np.asarray(w2, np.uint8)
        w2 = w2[None, :] if w2.ndim == 1 else w2
    if w64 is not None:
        w64 = np.asarray(w64, np.uint64)
        w64 = w64[None, :] if w64.ndim == 1 else w64
    B = w2.shape[0] if w2 is not None else w64.shape[0]
    w2 = w2 if w2 is not None else np.zeros((B, 0), np.uint8)
    w64 = w64 if w64 is not None else np.zeros((B, 0), np.uint64)
    assert w2.shape[0] == w64.shape[0] == B
    return w2, w64, B


def _sizes(prog, wc):
    """(z64, gf2) wire array sizes that hold every index the program names (SizeHint may grow them, as in model())"""
    n64, n2 = int(wc[0]), int(wc[1])
    for dom, idx in ((DOM_GF2, ("dst", "a", "b")), (DOM_Z64, ("dst", "a", "b"))):
        sel = prog[prog["domain"] == dom]
        if len(sel):
            m = max(int(sel[f].max()) for f in idx) + 1
            if dom == DOM_GF2:
                n2 = max(n2, m)
            else:
                n64 = max(n64, m)
    b2a = prog[prog["domain"] == DOM_B2A]
    if len(b2a):
        n64 = max(n64, int(b2a["dst"].max()) + 1)
        n2 = max(n2, int(b2a["a"].max()) + 64)
    hint = prog[prog["domain"] == DOM_SIZEHINT]
    if len(hint):
        n64, n2 = max(n64, int(hint["a"].max())), max(n2, int(hint["b"].max()))
    return n64, n2


def _bits(x: int, B: int) -> np.ndarray:
    """bool[B] of the bits of x"""
    nb = (B + 7) // 8
    return np.unpackbits(np.frombuffer(x.to_bytes(nb, "little"), np.uint8), bitorder="little")[:B].astype(bool)


def _int_columns(w2: np.ndarray):
    """the witness columns of [B][n] bytes as ints of B bits (non-zero byte -> 1)"""
    B, n = w2.shape
    if not n or not B:
        return [0] * n
    packed = np.packbits(w2 != 0, axis=0, bitorder="little")  # [ceil(B/8)][n]
    return [int.from_bytes(packed[:, i].tobytes(), "little") for i in range(n)]


def evaluate(prog, wc, w2, w64=None, gf2_cols=None):
    """op after op, every witness at once (gf2_cols: return only these GF(2) wires)"""
    prog = np.asarray(prog)
    w2, w64, B = _witnesses(w2, w64)
    n64, n2 = int(wc[0]), int(wc[1])
    N64, N2 = _sizes(prog, wc)
    ALL = (1 << B) - 1
    zero64 = np.zeros(B, np.uint64)
    v2, v64 = [0] * N2, [zero64] * N64
    cols2 = _int_columns(w2)
    i2 = i64 = 0
    n_failed = np.zeros(B, np.int64)
    first = np.full(B, -1, np.int64)

    def fail(i, m):
        n_failed[m] += 1
        first[m & (first < 0)] = i

    with np.errstate(over="ignore"):
        for i, (dom, opc, _r, d, a, b, imm) in enumerate(prog.tolist()):
            if dom == DOM_GF2:
                if opc == OP_INPUT:
                    v2[d] = cols2[i2]
                    i2 += 1
                elif opc in (OP_ADD, OP_SUB):
                    v2[d] = v2[a] ^ v2[b]
                elif opc in (OP_ADDCONST, OP_SUBCONST):
                    v2[d] = v2[a] ^ (ALL if imm & 1 else 0)
                elif opc == OP_MUL:
                    v2[d] = v2[a] & v2[b]
                elif opc == OP_MULCONST:
                    v2[d] = v2[a] if imm & 1 else 0
                elif opc == OP_CONST:
                    v2[d] = ALL if imm & 1 else 0
                elif opc == OP_ASSERTZERO:
                    if v2[a]:
                        fail(i, _bits(v2[a], B))
                else:
                    raise ValueError(f"op {i}: no cleartext value (opcode {opc})")
            elif dom == DOM_Z64:
                if opc == OP_INPUT:
                    v64[d] = w64[:, i64].copy()
                    i64 += 1
                elif opc == OP_ADD:
                    v64[d] = v64[a] + v64[b]
                elif opc == OP_SUB:
                    v64[d] = v64[a] - v64[b]
                elif opc == OP_ADDCONST:
                    v64[d] = v64[a] + np.uint64(imm)
                elif opc == OP_SUBCONST:
                    v64[d] = v64[a] - np.uint64(imm)
                elif opc == OP_MUL:
                    v64[d] = v64[a] * v64[b]
                elif opc == OP_MULCONST:
                    v64[d] = v64[a] * np.uint64(imm)
                elif opc == OP_CONST:
                    v64[d] = np.full(B, imm, np.uint64)
                elif opc == OP_ASSERTZERO:
                    m = v64[a] != 0
                    if m.any():
                        fail(i, m)
                else:
                    raise ValueError(f"op {i}: no cleartext value (opcode {opc})")
            elif dom == DOM_B2A:
                r = zero64.copy()
                for k in range(64):
                    if v2[a + k]:
                        r |= _bits(v2[a + k], B).astype(np.uint64) << np.uint64(k)
                v64[d] = r
            # (DOM_SIZEHINT: the arrays were sized for it up front)
    cols = range(n2) if gf2_cols is None else [int(w) for w in gf2_cols]
    gf2 = np.zeros((B, len(cols)), np.uint8)
    if len(cols) and B:
        nb = (B + 7) // 8
        packed = np.frombuffer(b"".join(v2[w].to_bytes(nb, "little") for w in cols), np.uint8).reshape(len(cols), nb)
        gf2 = np.ascontiguousarray(np.unpackbits(packed, axis=1, bitorder="little")[:, :B].T)
    z64 = np.stack(v64[:n64], axis=1) if n64 else np.zeros((B, 0), np.uint64)
    return gf2, z64, n_failed, first


# ---------------------------------------------------------------- layer by layer
_READS_A = (OP_ADD, OP_SUB, OP_MUL, OP_ADDCONST, OP_SUBCONST, OP_MULCONST, OP_ASSERTZERO)
_READS_B = (OP_ADD, OP_SUB, OP_MUL)


def _keys(prog):
    """per op: the (domain-tagged) wire keys it reads (a, b; -1 for none) and writes (-1 for none)"""
    dom = prog["domain"].astype(np.int64)
    opc = prog["opcode"]
    tag = lambda w: w.astype(np.int64) * 2 + dom  # noqa: E731  (GF(2) even, Z64 odd)
    real = (dom == DOM_GF2) | (dom == DOM_Z64)
    ra = np.where(real & np.isin(opc, _READS_A), tag(prog["a"]), -1)
    rb = np.where(real & np.isin(opc, _READS_B), tag(prog["b"]), -1)
    wr = np.where(real & (opc != OP_ASSERTZERO), tag(prog["dst"]), -1)
    return ra, rb, wr


def _first_conflict(ra, rb, wr, lo, end):
    """the first op in [lo, end) that reads or writes a wire an earlier op of [lo, end) writes (end if none)"""
    w = wr[lo:end]
    pos = np.nonzero(w >= 0)[0]
    if not len(pos):
        return end
    uk, ui = np.unique(w[pos], return_index=True)
    firstpos = pos[ui]  # (first write of each key in the window)
    best = end - lo
    for keys in (ra[lo:end], rb[lo:end], w):
        at = np.nonzero(keys >= 0)[0]
        if not len(at):
            continue
        j = np.searchsorted(uk, keys[at])
        j = np.minimum(j, len(uk) - 1)
        hit = (uk[j] == keys[at]) & (firstpos[j] < at)
        if hit.any():
            best = min(best, int(at[hit][0]))
    return lo + best


def layers(prog):
    """contiguous op ranges [lo, hi) in which no op reads or rewrites a wire that an earlier op of the range writes: each range can be
    evaluated at once, every read before every write"""
    prog = np.asarray(prog)
    if np.any(prog["domain"] == DOM_B2A) or np.any((prog["opcode"] == OP_RANDOM) & (prog["domain"] <= DOM_Z64)):
        raise ValueError("evaluate_layers: B2A and Random ops are not supported (use evaluate)")
    ra, rb, wr = _keys(prog)
    n, lo, L, out = len(prog), 0, 64, []
    while lo < n:
        while True:
            end = min(n, lo + L)
            hi = _first_conflict(ra, rb, wr, lo, end)
            if hi < end or end == n:
                break
            L *= 2
        out.append((lo, hi))
        L = max(64, 2 * (hi - lo))
        lo = hi
    return out


def evaluate_layers(prog, wc, w2, w64=None, bounds=None):
    """evaluate() one layer at a time (layers(prog) unless `bounds` are given): GF(2) values bit-sliced in uint64 words [wire][W],
    Z64 values [wire][B].  For layered circuits (circuits.layered_gf2 / layered_z64) with a few hundred layers."""
    prog = np.asarray(prog)
    w2, w64, B = _witnesses(w2, w64)
    n64, n2 = int(wc[0]), int(wc[1])
    N64, N2 = _sizes(prog, wc)
    W = max((B + 63) // 64, 1)
    allw = np.full(W, M64, np.uint64)
    if B % 64:
        allw[-1] = np.uint64((1 << (B % 64)) - 1)
    V2 = np.zeros((N2, W), np.uint64)
    V64 = np.zeros((N64, B), np.uint64)
    # witness columns bit-sliced: [n][W]
    n_in2 = w2.shape[1]
    packed = np.zeros((W * 8, n_in2), np.uint8)
    if B:
        packed[:(B + 7) // 8] = np.packbits(w2 != 0, axis=0, bitorder="little")
    win = np.ascontiguousarray(packed.T).view("<u8").reshape(n_in2, W)
    i2 = i64 = 0
    n_failed = np.zeros(B, np.int64)
    first = np.full(B, -1, np.int64)

    def unbits(rows):  # [k][W] words -> bool [k][B]
        return np.unpackbits(np.ascontiguousarray(rows).view(np.uint8), axis=1, bitorder="little")[:, :B].astype(bool)

    def fail(idx, m):  # op indices [k] (program order), failing witnesses bool [k][B]
        nonlocal first
        if not m.any():
            return
        n_failed[:] += m.sum(0)
        any_f = m.any(0)
        at = idx[np.argmax(m, axis=0)]
        sel = any_f & (first < 0)
        first[sel] = at[sel]

    for lo, hi in (bounds if bounds is not None else layers(prog)):
        L = prog[lo:hi]
        idx = np.arange(lo, hi)
        dom, opc = L["domain"], L["opcode"]
        d, a, b = L["dst"].astype(np.int64), L["a"].astype(np.int64), L["b"].astype(np.int64)
        c1 = (L["imm"] & np.uint64(1)).astype(bool)
        with np.errstate(over="ignore"):
            # GF(2)
            g = dom == DOM_GF2
            if g.any():
                writes = []
                m = g & (opc == OP_INPUT)
                if m.any():
                    k = int(m.sum())
                    writes.append((d[m], win[i2:i2 + k]))
                    i2 += k
                m = g & np.isin(opc, (OP_ADD, OP_SUB, OP_MUL))
                if m.any():
                    va, vb = V2[a[m]], V2[b[m]]
                    writes.append((d[m], np.where((opc[m] == OP_MUL)[:, None], va & vb, va ^ vb)))
                m = g & np.isin(opc, (OP_ADDCONST, OP_SUBCONST))
                if m.any():
                    writes.append((d[m], V2[a[m]] ^ np.where(c1[m][:, None], allw, np.uint64(0))))
                m = g & (opc == OP_MULCONST)
                if m.any():
                    writes.append((d[m], np.where(c1[m][:, None], V2[a[m]], np.uint64(0))))
                m = g & (opc == OP_CONST)
                if m.any():
                    writes.append((d[m], np.where(c1[m][:, None], allw, np.uint64(0))))
                m = g & (opc == OP_ASSERTZERO)
                if m.any():
                    fail(idx[m], unbits(V2[a[m]] & allw))
                for dst, val in writes:
                    V2[dst] = val & allw
            # Z64
            z = dom == DOM_Z64
            if z.any():
                writes = []
                m = z & (opc == OP_INPUT)
                if m.any():
                    k = int(m.sum())
                    writes.append((d[m], w64[:, i64:i64 + k].T))
                    i64 += k
                imm = L["imm"][:, None]
                for op, f in ((OP_ADD, lambda x, y: x + V64[y]), (OP_SUB, lambda x, y: x - V64[y]), (OP_MUL, lambda x, y: x * V64[y])):
                    m = z & (opc == op)
                    if m.any():
                        writes.append((d[m], f(V64[a[m]], b[m])))
                for op, f in ((OP_ADDCONST, np.add), (OP_SUBCONST, np.subtract), (OP_MULCONST, np.multiply)):
                    m = z & (opc == op)
                    if m.any():
                        writes.append((d[m], f(V64[a[m]], imm[m])))
                m = z & (opc == OP_CONST)
                if m.any():
                    writes.append((d[m], np.broadcast_to(imm[m], (int(m.sum()), B))))
                m = z & (opc == OP_ASSERTZERO)
                if m.any():
                    fail(idx[m], V64[a[m]] != 0)
                for dst, val in writes:
                    V64[dst] = val
    gf2 = np.zeros((B, n2), np.uint8)
    for k in range(B):
        gf2[k] = (V2[:n2, k // 64] >> np.uint64(k % 64)) & np.uint64(1)
    return gf2, np.ascontiguousarray(V64[:n64].T), n_failed, first
