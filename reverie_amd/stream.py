"""Host-side mirror of the streaming prover (include/reverie_amd.h: rv_stream_*).

The reference's README promises a streaming interface (/root/reference/README.md:14); its `Proof::new`
(src/proof/mod.rs:119-222) takes the whole gate list at once.  `StreamingProver` takes the gate list in pieces, twice:

    sp = StreamingProver((z64_wires, gf2_wires), seeds=seeds)
    for ops, w2, w64 in pieces: sp.feed(ops, w2, w64)     # pass 1
    comm = sp.commit()
    for ops, w2, w64 in pieces: sp.feed(ops, w2, w64)     # pass 2 (the same ops again)
    proof = sp.finish()                                    # == Proof.new(all ops, all witness, seeds=seeds)

Device memory is bounded by the wire counts, one piece's working set and the proof; everything runs through the C-ABI.
`StreamingVerifier` checks a proof against a gate list fed in pieces, and `StreamingEvaluator` evaluates one in the clear.
`StreamingBatchProver` / `StreamingBatchVerifier` prove or verify several witnesses / proofs of one statement over one fed list.

Every class and one-shot function here takes `device_compile` (default False): the stream's all-GF(2) pieces are then compiled on the
GPU (RV_COMPILE_DEVICE: rv_stream_set_compile_flags / rv_eval_stream_set_compile_flags) instead of on host worker threads; pieces with
Z64, B2A or SizeHint ops, and pieces with an error in them, are still compiled on the host.  Proofs, answers and values are the same.
With `device_z64=True` as well (RV_COMPILE_DEVICE_Z64; a ValueError without `device_compile`) Z64 and mixed pieces are compiled on the
GPU too: only pieces with a B2A op or an error in them are left to the host.  With `device_b2a=True` on top of both
(RV_COMPILE_DEVICE_B2A; a ValueError without the other two) pieces with B2A ops are compiled on the GPU as well: every piece goes to
the device compiler, and only one with an error in it comes back to the host compiler, which reports it.

Wherever an op list is taken -- every `feed`, every one-shot function -- it may also be a torch tensor in GPU memory holding packed
rv_op records (what `Circuit.from_device_ops` accepts; on the context's device, or it is an error).  The ops are then fed from where
they are (rv_stream_feed_device / rv_eval_stream_feed_device): with `device_compile` an all-GF(2) piece never reaches the host, and a
piece the host compiler has to read is copied down alone.  Results are the same bytes.

Wherever a witness is taken it may be a pair of torch tensors in GPU memory (`proof._device_witness`: uint8 / bool [n] or [B][n],
int64 / uint64 [m] or [B][m], rows may be strided): the stream reads them where they lie (rv_stream_feed_wdev /
rv_eval_stream_feed_wdev), with host or device ops alike.  `finish(device=True)` (one-shot: `device_proof=True`) leaves the proof in a
torch uint8 GPU tensor and returns a `DeviceProof`; the verifiers take a `DeviceProof` or a uint8 GPU tensor wherever they take proof
bytes and read it in place (rv_stream_verify_begin_device).  Proofs, answers and values are the same bytes either way.

The whole-list one-shot functions also take `prune` (default False): the ops no assertion depends on are dropped first
(`prune.prune_ops`), then `compact_wires` runs if asked for, and the stream info (or `info`) receives "prune".  The proof is then the
proof of the pruned list -- prover and verifier must both pass prune=True.  The `*_streaming_pieces` functions take `prune` too:
the pieces are then pruned in windows (`prune.prune_pieces`, DESIGN §23.8: the source is read twice more, one of them backwards, so
the pieces' callable needs `.backwards`), before `compact_wires`, and the result is the same.

The whole-list one-shot functions take `fold` (default False) as well: constants are folded first (`fold.fold_ops`), before
`prune` and `compact_wires`, and the info receives "fold".  The proof is the proof of the folded list -- prover and verifier must both
pass fold=True.  The `*_streaming_pieces` functions refuse it: a read of an index no earlier op wrote is known 0, and a window's
unwritten index is not the list's.  `fold.fold_pieces(pieces, wire_counts)` is the windowed form: it carries the known
values from window to window and returns pieces these functions take, `prune=True` and `compact_wires=True` on top included.

The one-shot functions take `compact_wires` (default False): the whole op list is first renumbered by liveness (`compact.compact_wires`,
DESIGN §17) -- on the host for host ops, by kernels for a GPU tensor -- and the stream begins with the new, smaller wire counts, so an
SSA-numbered list no longer costs a wire-store row per gate.  Proofs and answers are the same bytes; the wire values
`evaluate_streaming` returns are those of the new indices (an op's renumbered `dst` is where its value lives), and the stream info
carries rv_compact_info under "compact".  The feeding classes are unchanged: a caller who feeds in pieces compacts the whole list first
-- or, with the `*_streaming_pieces` functions, passes `compact_wires=True`: the pieces are then compacted in windows
(`compact.compact_pieces`, DESIGN §17.5: the source is read once or twice more), nothing is sized by the whole list, and the result is
the same.
"""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib
from . import compact as _compact
from .ops import OP_DTYPE, TOTAL_REPS, program
from .proof import Context, DeviceProof, Evaluation, Proof, _device_bytes, _device_ops, _device_witness, _is_device_ops, _ptr


def _ops_ctx(ops, ctx: Optional[Context]) -> Context:
    """the context of a one-shot call; an op tensor that is not in GPU memory is refused before a context is made"""
    return _device_ops(ops, ctx, "a stream of device ops")[2] if _is_device_ops(ops) else ctx or Context.default()


def _compacted(ops, wire_counts, ctx: Context, wanted: bool, prune: bool = False, fold: bool = False):
    """the op list and wire counts a one-shot call streams, and (rv_compact_info, rv_prune_info, rv_fold_info) -- None where
    compact_wires / prune / fold was not asked for.  Folding comes first, then pruning (against the assertions: a stream has no
    outputs), then compaction."""
    pinfo = cinfo = finfo = None
    if fold:
        from .fold import fold_ops

        ops, finfo = fold_ops(ops, wire_counts, ctx=ctx)
    if prune:
        from .prune import prune_ops

        ops, pinfo, _ = prune_ops(ops, wire_counts, ctx=ctx)
    if wanted:
        ops, wire_counts, cinfo = _compact.compact_wires(ops, wire_counts, ctx)
    return ops, wire_counts, (cinfo, pinfo, finfo)


class _Owned:
    """the pruner and the compactor a `*_streaming_pieces` call made and has to close"""

    def __init__(self, *objs):
        self.objs = [o for o in objs if o is not None]

    def close(self) -> None:
        for o in self.objs:
            o.close()


def _compacted_pieces(pieces, wire_counts, ctx: Optional[Context], wanted: bool, prune: bool = False, fold: bool = False):
    """the pieces and wire counts a `*_streaming_pieces` call streams, (rv_compact_info, rv_prune_info) (None where compact_wires /
    prune was not asked for) and what this call made and has to close (None: it made nothing -- pieces that a caller pruned or
    compacted are the caller's).  Pruning (in windows, against the assertions: `prune.prune_pieces`) comes first, then compaction
    over the pruned pieces.  fold is refused: the whole-list functions fold."""
    if fold:
        raise ValueError("fold=True needs the whole list: a read of an index no earlier op wrote is known 0, and a window's unwritten index "
                         "is not the list's -- fold the list first (fold.fold_ops), use the whole-list function, or fold the pieces in "
                         "windows with the state carried from one to the next: fold.fold_pieces(pieces, wire_counts)[0] is a source of "
                         "pieces that these functions take as it is (prover and verifier both)")
    if not wanted and not prune:
        return pieces, wire_counts, None, None
    if not callable(pieces):
        raise TypeError("compact_wires and prune read the pieces more than once: pass a callable that returns a fresh iterator")
    pinfo = cinfo = pruner = compactor = None
    if prune:
        from .prune import prune_pieces

        pieces, pinfo = prune_pieces(pieces, wire_counts, ctx=ctx)
        pruner = pieces.pruner
    if wanted:
        try:
            wire_counts, pieces, cinfo = _compact.compact_pieces(pieces, wire_counts, ctx)
        except BaseException:
            if pruner is not None:
                pruner.close()
            raise
        compactor = pieces.compactor
    return pieces, wire_counts, (cinfo, pinfo), _Owned(pruner, compactor)


def _with_compact(info: dict, cinfo) -> dict:
    """cinfo: rv_compact_info, or _compacted's tuple"""
    cinfo, pinfo, finfo = (tuple(cinfo) + (None,))[:3] if isinstance(cinfo, tuple) else (cinfo, None, None)
    if finfo is not None:
        info["fold"] = finfo
    if pinfo is not None:
        info["prune"] = pinfo
    if cinfo is not None:
        info["compact"] = cinfo
    return info


def _feed(handle, ctx: Context, ops, g, n_g: int, z, n_z: int, entry: str = "rv_stream_feed"):
    """one feed of host ops (anything `program` takes) or of a torch GPU tensor of packed rv_op records (the _device entry point)"""
    if _is_device_ops(ops):
        d_ops, n_ops, _ = _device_ops(ops, ctx, "a feed of device ops")
        _lib.check(getattr(_lib.lib(), entry + "_device")(handle, C.c_void_p(d_ops), C.c_size_t(n_ops), _ptr(g), C.c_size_t(n_g), _ptr(z), C.c_size_t(n_z)))
        return
    ops = program(ops) if len(ops) else np.zeros(0, OP_DTYPE)
    _lib.check(getattr(_lib.lib(), entry)(handle, _ptr(ops), C.c_size_t(len(ops)), _ptr(g), C.c_size_t(n_g), _ptr(z), C.c_size_t(n_z)))


def _wdev(wit_gf2, wit_z64, ctx: Optional[Context], what: str, batched: bool):
    """The witnesses of a feed when they are torch GPU tensors: `_device_witness`'s (descriptor, batch, tensors, context), or None for
    host witnesses.  A torch tensor in host memory, and a pair that is half host and half device, is a TypeError -- raised before any
    context is made (ctx None: the default one)."""
    import sys

    torch = sys.modules.get("torch")
    if torch is not None:
        for t in (wit_gf2, wit_z64):
            if isinstance(t, torch.Tensor) and t.device.type != "cuda":
                raise TypeError(f"{what}: a witness tensor must be in GPU memory (pass host witnesses as arrays or sequences)")
    return _device_witness(wit_gf2, wit_z64, ctx, what, batched)


def _rows_batched(wit_gf2, wit_z64, batch: int) -> bool:
    """a batch of one may pass its witness as [n]"""
    return not (batch == 1 and all(getattr(t, "ndim", 2) == 1 for t in (wit_gf2, wit_z64) if hasattr(t, "data_ptr")))


def _feed_wdev(handle, ctx: Context, ops, dw, entry: str = "rv_stream_feed"):
    """one feed with witnesses in GPU memory (`dw` from `_wdev`); the ops from the host or from a torch GPU tensor"""
    if _is_device_ops(ops):
        d_ops, n_ops, _ = _device_ops(ops, ctx, "a feed of device ops")
        ptr, on_device = C.c_void_p(d_ops), 1
    else:
        ops = program(ops) if len(ops) else np.zeros(0, OP_DTYPE)
        ptr, n_ops, on_device = _ptr(ops), len(ops), 0
    _lib.check(getattr(_lib.lib(), entry + "_wdev")(handle, ptr, C.c_size_t(n_ops), C.c_int(on_device), C.byref(dw[0])))


def _device_proof_bytes(proof, ctx: Optional[Context], what: str):
    """(pointer, length, the object to keep alive) of a proof in GPU memory -- a bincode-form DeviceProof or a uint8 GPU tensor -- or
    None for host bytes"""
    import sys

    torch = sys.modules.get("torch")
    if isinstance(proof, DeviceProof):
        if proof.lens is not None:
            raise TypeError(f"{what} takes bincode-form proofs; a sections-form DeviceProof verifies on its own")
        if ctx is not None and ctx.device != proof.ctx.device:
            raise ValueError(f"the proof is on device {proof.ctx.device}, the context on device {ctx.device}")
        return proof._ptr, proof._len, proof
    if torch is not None and isinstance(proof, torch.Tensor):
        ptr, n, _ = _device_bytes(proof, ctx, what)
        return ptr, n, proof
    return None


def _check_device_z64(device_compile: bool, device_z64: bool, device_b2a: bool = False):
    if device_z64 and not device_compile:
        raise ValueError("device_z64=True needs device_compile=True")
    if device_b2a and not (device_compile and device_z64):
        raise ValueError("device_b2a=True needs device_compile=True and device_z64=True")


def _device_flags(device_compile: bool, device_z64: bool, device_b2a: bool = False) -> int:
    _check_device_z64(device_compile, device_z64, device_b2a)
    return (_lib.RV_COMPILE_DEVICE if device_compile else 0) | (_lib.RV_COMPILE_DEVICE_Z64 if device_z64 else 0) | \
        (_lib.RV_COMPILE_DEVICE_B2A if device_b2a else 0)


def _set_device_compile(handle, device_compile: bool, device_z64: bool = False, device_b2a: bool = False, setter: str = "rv_stream_set_compile_flags"):
    """a new stream follows its context's flags; device_compile=True asks for the device compiler whatever they are (device_z64: for
    Z64 and mixed pieces too; device_b2a: for pieces with B2A ops too, that is for every piece)"""
    if device_compile:
        _lib.check(getattr(_lib.lib(), setter)(handle, C.c_uint32(_device_flags(device_compile, device_z64, device_b2a))))


@contextlib.contextmanager
def _ctx_device_compile(ctx: Context, device_compile: bool, device_z64: bool = False, device_b2a: bool = False):
    """The one-shot calls of the library follow their context's compile flags, so device_compile=True sets RV_COMPILE_DEVICE (and
    device_z64=True RV_COMPILE_DEVICE_Z64, device_b2a=True RV_COMPILE_DEVICE_B2A) on `ctx`
    for the duration of the call and puts back what Context.set_compile_flags last set.  The context is shared state: another
    thread's cold rv_prove_ops / rv_verify_ops compiles on the same context meanwhile use the device compiler too (same results),
    and flags set through the C API behind Context's back are not seen here.  A caller who minds either sets the flag on the
    context once, or uses the Streaming* classes, whose flag lives on the stream handle."""
    before = getattr(ctx, "compile_flags", 0)
    want = before | _device_flags(device_compile, device_z64, device_b2a)
    if want != before:
        ctx.set_compile_flags(want)
        try:
            yield
        finally:
            ctx.set_compile_flags(before)
    else:
        yield


class StreamingProver:
    def __init__(self, wire_counts: Tuple[int, int], seeds=None, max_chunk_ops: int = 0, ctx: Optional[Context] = None,
                 device_compile: bool = False, device_z64: bool = False, device_b2a: bool = False):
        _check_device_z64(device_compile, device_z64, device_b2a)
        self.ctx = ctx or Context.default()
        self.handle = C.c_void_p()
        s = None
        if seeds is not None:
            s = np.ascontiguousarray(np.frombuffer(bytes(seeds), np.uint8) if isinstance(seeds, (bytes, bytearray))
                                     else np.asarray(seeds, dtype=np.uint8)).reshape(TOTAL_REPS, 16)
        _lib.check(_lib.lib().rv_stream_begin(self.ctx.handle, C.c_size_t(int(wire_counts[0])), C.c_size_t(int(wire_counts[1])), _ptr(s),
                                              C.c_size_t(max_chunk_ops), C.byref(self.handle)))
        _set_device_compile(self.handle, device_compile, device_z64, device_b2a)

    def feed(self, ops, wit_gf2: Sequence[int] = (), wit_z64: Sequence[int] = ()):
        dw = _wdev(wit_gf2, wit_z64, getattr(self, "ctx", None), "StreamingProver.feed", batched=False)
        if dw is not None:
            return _feed_wdev(self.handle, self.ctx, ops, dw)
        g = np.ascontiguousarray(np.asarray(wit_gf2, dtype=np.uint8))
        z = np.ascontiguousarray(np.asarray(wit_z64, dtype=np.uint64))
        _feed(self.handle, self.ctx, ops, g, len(g), z, len(z))

    def same_cuts(self):
        """rv_stream_same_cuts: pass 2 will be fed in pass 1's pieces -- pass 1 keeps the last chunks' transcripts within
        RV_STREAM_KEEP_MB and pass 2 takes their openings from them instead of running them again"""
        _lib.check(_lib.lib().rv_stream_same_cuts(self.handle))

    def commit(self) -> bytes:
        comm = np.zeros(32, np.uint8)
        _lib.check(_lib.lib().rv_stream_commit(self.handle, _ptr(comm)))
        return comm.tobytes()

    def finish(self, device: bool = False) -> "Proof | DeviceProof":
        """the proof; device=True: left in a torch uint8 GPU tensor (rv_stream_finish_device), as a DeviceProof -- the same bytes"""
        if device:
            import torch

            want = self.info["proof_bytes"]
            out = torch.empty(want, dtype=torch.uint8, device=f"cuda:{self.ctx.device}")
            n = C.c_size_t()
            _lib.check(_lib.lib().rv_stream_finish_device(self.handle, C.c_void_p(out.data_ptr()), C.c_size_t(want), C.byref(n)))
            return DeviceProof(out[:n.value], ctx=self.ctx)
        out, n = C.c_void_p(), C.c_size_t()
        _lib.check(_lib.lib().rv_stream_finish(self.handle, C.byref(out), C.byref(n)))
        return Proof(_owned=(C.c_void_p(out.value), n.value))

    @property
    def info(self) -> dict:
        si = _lib.StreamInfo()
        _lib.check(_lib.lib().rv_stream_get_info(self.handle, C.byref(si)))
        return {n: int(getattr(si, n)) for n, _ in si._fields_}

    def close(self):
        if self.handle:
            if self.ctx.handle:
                _lib.lib().rv_stream_abort(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def prove_streaming(ops, wit_gf2, wit_z64, wire_counts: Tuple[int, int], seeds=None, max_chunk_ops: int = 0,
                    ctx: Optional[Context] = None, device_compile: bool = False, device_z64: bool = False, device_b2a: bool = False,
                    device_proof: bool = False, compact_wires: bool = False, prune: bool = False, fold: bool = False) -> Tuple[Proof, dict]:
    """rv_prove_streaming: both passes over an op array in host memory -> (Proof, stream info).  A torch GPU tensor of ops, witnesses
    that are torch GPU tensors or device_proof=True (-> a DeviceProof): the same through rv_stream_begin / the feeds / the finish.
    compact_wires: the list is renumbered by liveness first and the stream begins with the new counts (the same proof)."""
    _check_device_z64(device_compile, device_z64, device_b2a)
    on_device = _wdev(wit_gf2, wit_z64, ctx, "prove_streaming", batched=False) is not None  # (refuses before a context is made)
    ctx = _ops_ctx(ops, ctx)
    ops, wire_counts, cinfo = _compacted(ops, wire_counts, ctx, compact_wires, prune, fold)
    if _is_device_ops(ops) or on_device or device_proof:
        sp = StreamingProver(wire_counts, seeds, max_chunk_ops, ctx, device_compile, device_z64, device_b2a)
        try:
            sp.same_cuts()  # (the same ops, cut by the same rule in both passes)
            sp.feed(ops, wit_gf2, wit_z64)
            sp.commit()
            sp.feed(ops, wit_gf2, wit_z64)
            return sp.finish(device=device_proof), _with_compact(sp.info, cinfo)
        finally:
            sp.close()
    ops = program(ops) if len(ops) else np.zeros(0, OP_DTYPE)
    g = np.ascontiguousarray(np.asarray(wit_gf2, dtype=np.uint8))
    z = np.ascontiguousarray(np.asarray(wit_z64, dtype=np.uint64))
    s = None
    if seeds is not None:
        s = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint8)).reshape(TOTAL_REPS, 16)
    out, n = C.c_void_p(), C.c_size_t()
    si = _lib.StreamInfo()
    with _ctx_device_compile(ctx, device_compile, device_z64, device_b2a):
        _lib.check(_lib.lib().rv_prove_streaming(ctx.handle, _ptr(ops), C.c_size_t(len(ops)), C.c_size_t(int(wire_counts[0])),
                                                 C.c_size_t(int(wire_counts[1])), _ptr(g), C.c_size_t(len(g)), _ptr(z), C.c_size_t(len(z)), _ptr(s),
                                                 C.c_size_t(max_chunk_ops), C.byref(out), C.byref(n), C.byref(si)))
    return Proof(_owned=(C.c_void_p(out.value), n.value)), _with_compact({k: int(getattr(si, k)) for k, _ in si._fields_}, cinfo)


class StreamingVerifier:
    """Proof::verify with bounded device memory: the ops are fed in pieces, once (rv_stream_verify_begin / feed / finish).

        sv = StreamingVerifier((z64_wires, gf2_wires), proof)
        for ops in pieces: sv.feed(ops)
        ok = sv.finish()            # == proof.verify(all ops, (z64_wires, gf2_wires))
    """

    def __init__(self, wire_counts: Tuple[int, int], proof, max_chunk_ops: int = 0, ctx: Optional[Context] = None,
                 device_compile: bool = False, device_z64: bool = False, device_b2a: bool = False):
        _check_device_z64(device_compile, device_z64, device_b2a)
        self.handle = C.c_void_p()
        dev = _device_proof_bytes(proof, ctx, "StreamingVerifier")
        self.ctx = ctx or (proof.ctx if isinstance(proof, DeviceProof) else Context.default())
        if dev is not None:  # read in place: the tensor is kept alive for the stream's life
            self._proof = dev[2]
            _lib.check(_lib.lib().rv_stream_verify_begin_device(self.ctx.handle, C.c_size_t(int(wire_counts[0])), C.c_size_t(int(wire_counts[1])),
                                                                C.c_void_p(dev[0]), C.c_size_t(dev[1]), C.c_size_t(max_chunk_ops), C.byref(self.handle)))
            _set_device_compile(self.handle, device_compile, device_z64, device_b2a)
            return
        self._proof = proof if isinstance(proof, Proof) else Proof(bytes(proof))  # (kept alive: the stream reads it until finish)
        buf, n = self._proof._buffer()
        _lib.check(_lib.lib().rv_stream_verify_begin(self.ctx.handle, C.c_size_t(int(wire_counts[0])), C.c_size_t(int(wire_counts[1])), buf,
                                                     C.c_size_t(n), C.c_size_t(max_chunk_ops), C.byref(self.handle)))
        _set_device_compile(self.handle, device_compile, device_z64, device_b2a)

    def feed(self, ops):
        _feed(self.handle, self.ctx, ops, None, 0, None, 0)

    def finish(self, strict: bool = True) -> bool:
        ok = C.c_int()
        _lib.check(_lib.lib().rv_stream_verify_finish(self.handle, C.c_uint32(0 if strict else _lib.RV_VERIFY_REFERENCE_COMPAT), C.byref(ok)))
        return bool(ok.value)

    info = StreamingProver.info
    close = StreamingProver.close

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def verify_streaming(ops, wire_counts: Tuple[int, int], proof, strict: bool = True, max_chunk_ops: int = 0,
                     ctx: Optional[Context] = None, device_compile: bool = False, device_z64: bool = False, device_b2a: bool = False,
                     compact_wires: bool = False, prune: bool = False, fold: bool = False) -> Tuple[bool, dict]:
    """rv_verify_streaming: one pass over an op array in host memory -> (ok, stream info).  A torch GPU tensor of ops: the same through
    rv_stream_verify_begin / rv_stream_feed_device / rv_stream_verify_finish.  compact_wires: as in prove_streaming (the same answer)."""
    _check_device_z64(device_compile, device_z64, device_b2a)
    on_device = _device_proof_bytes(proof, ctx, "verify_streaming") is not None
    if on_device and ctx is None and isinstance(proof, DeviceProof):
        ctx = proof.ctx
    ctx = _ops_ctx(ops, ctx)
    ops, wire_counts, cinfo = _compacted(ops, wire_counts, ctx, compact_wires, prune, fold)
    if _is_device_ops(ops) or on_device:
        sv = StreamingVerifier(wire_counts, proof, max_chunk_ops, ctx, device_compile, device_z64, device_b2a)
        try:
            sv.feed(ops)
            return sv.finish(strict), _with_compact(sv.info, cinfo)
        finally:
            sv.close()
    ops = program(ops) if len(ops) else np.zeros(0, OP_DTYPE)
    pr = proof if isinstance(proof, Proof) else Proof(bytes(proof))
    buf, n = pr._buffer()
    ok = C.c_int()
    si = _lib.StreamInfo()
    with _ctx_device_compile(ctx, device_compile, device_z64, device_b2a):
        _lib.check(_lib.lib().rv_verify_streaming(ctx.handle, _ptr(ops), C.c_size_t(len(ops)), C.c_size_t(int(wire_counts[0])), C.c_size_t(int(wire_counts[1])),
                                                  buf, C.c_size_t(n), C.c_uint32(0 if strict else _lib.RV_VERIFY_REFERENCE_COMPAT), C.c_size_t(max_chunk_ops),
                                                  C.byref(ok), C.byref(si)))
    return bool(ok.value), _with_compact({k: int(getattr(si, k)) for k, _ in si._fields_}, cinfo)


def _batch_seeds(seeds, batch: int):
    if seeds is None:
        return None
    a = np.frombuffer(bytes(seeds), np.uint8) if isinstance(seeds, (bytes, bytearray)) else np.asarray(seeds, dtype=np.uint8)
    return np.ascontiguousarray(a).reshape(batch, TOTAL_REPS, 16)


def _proof_array(proofs):
    """(kept objects, pointer array, length array) of Proof objects or bytes, read in place"""
    n = len(proofs)
    keep, ptrs, lens = [], (C.c_void_p * n)(), (C.c_size_t * n)()
    for i, p in enumerate(proofs):
        pr = p if isinstance(p, Proof) else Proof(bytes(p))
        buf, ln = pr._buffer()
        keep += [pr, buf]
        ptrs[i] = C.cast(buf, C.c_void_p).value
        lens[i] = ln
    return keep, ptrs, lens


def _info(si) -> dict:
    return {k: int(getattr(si, k)) for k, _ in si._fields_}


class StreamingBatchProver:
    """`batch` proofs of one statement over ONE streamed op list (rv_stream_begin_batch): each piece is compiled once per pass
    and proved for every witness.

        sp = StreamingBatchProver((z64_wires, gf2_wires), batch=B, seeds=seeds)   # seeds: [B][256][16] or None
        for ops, w2, w64 in pieces: sp.feed(ops, w2, w64)    # w2: [B][n], w64: [B][m] -- the elements these ops' Inputs consume
        comms = sp.commit()
        for ops, w2, w64 in pieces: sp.feed(ops, w2, w64)    # pass 2: the same ops and witnesses again
        proofs = sp.finish()                                  # proofs[b] == Proof.new(all ops, witness b, seeds=seeds[b])
    """

    def __init__(self, wire_counts: Tuple[int, int], batch: int, seeds=None, max_chunk_ops: int = 0, ctx: Optional[Context] = None,
                 device_compile: bool = False, device_z64: bool = False, device_b2a: bool = False):
        _check_device_z64(device_compile, device_z64, device_b2a)
        self.ctx = ctx or Context.default()
        self.batch = int(batch)
        self.handle = C.c_void_p()
        if self.batch < 1:
            raise ValueError("batch must be at least 1")
        s = _batch_seeds(seeds, self.batch)
        _lib.check(_lib.lib().rv_stream_begin_batch(self.ctx.handle, int(wire_counts[0]), int(wire_counts[1]), self.batch, _ptr(s),
                                                    int(max_chunk_ops), C.byref(self.handle)))
        _set_device_compile(self.handle, device_compile, device_z64, device_b2a)

    def feed(self, ops, wits_gf2=(), wits_z64=()):
        dw = _wdev(wits_gf2, wits_z64, getattr(self, "ctx", None), "StreamingBatchProver.feed", batched=_rows_batched(wits_gf2, wits_z64, self.batch))
        if dw is not None:
            if dw[1] != self.batch:
                raise ValueError(f"witnesses must be [batch={self.batch}][n]")
            return _feed_wdev(self.handle, self.ctx, ops, dw)
        g = _eval_wits(wits_gf2, self.batch, np.uint8)
        z = _eval_wits(wits_z64, self.batch, np.uint64)
        _feed(self.handle, self.ctx, ops, g, g.shape[1], z, z.shape[1])

    same_cuts = StreamingProver.same_cuts

    def commit(self) -> "list[bytes]":
        comms = np.zeros((self.batch, 32), np.uint8)
        _lib.check(_lib.lib().rv_stream_commit_batch(self.handle, _ptr(comms)))
        return [comms[b].tobytes() for b in range(self.batch)]

    def finish(self, device: bool = False) -> "list[Proof] | list[DeviceProof]":
        """the proofs; device=True: DeviceProof views of ONE torch uint8 GPU tensor (rv_stream_finish_batch_device; proof b at
        b * stride, stride = the proof length rounded up to 256), the same bytes"""
        if device:
            import torch

            want = self.info["proof_bytes"] // self.batch
            stride = (want + 255) & ~255
            out = torch.empty(self.batch * stride, dtype=torch.uint8, device=f"cuda:{self.ctx.device}")
            n = C.c_size_t()
            _lib.check(_lib.lib().rv_stream_finish_batch_device(self.handle, C.c_void_p(out.data_ptr()), C.c_size_t(stride), C.byref(n)))
            proofs = []
            for b in range(self.batch):  # (the call has waited for its stream)
                dp = DeviceProof.__new__(DeviceProof)
                dp.lens, dp._comm, dp.ctx = None, None, self.ctx
                dp.tensor = out[b * stride:b * stride + n.value]
                dp._ptr, dp._len = out.data_ptr() + b * stride, n.value
                proofs.append(dp)
            return proofs
        outs = (C.c_void_p * self.batch)()
        lens = (C.c_size_t * self.batch)()
        _lib.check(_lib.lib().rv_stream_finish_batch(self.handle, outs, lens))
        return [Proof(_owned=(C.c_void_p(outs[b]), int(lens[b]))) for b in range(self.batch)]

    info = StreamingProver.info
    close = StreamingProver.close

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def prove_streaming_batch(ops, wits_gf2, wits_z64, wire_counts: Tuple[int, int], seeds=None, max_chunk_ops: int = 0,
                          ctx: Optional[Context] = None, info: Optional[dict] = None, device_compile: bool = False, device_z64: bool = False, device_b2a: bool = False,
                          device_proof: bool = False, compact_wires: bool = False, prune: bool = False, fold: bool = False) -> "list[Proof]":
    """rv_prove_streaming_batch: both passes over an op array in host memory for the witnesses wits_gf2 [B][n] / wits_z64
    [B][m] (B from whichever of the two is 2-D; the other may be []); seeds [B][256][16] or None.  `info` (a dict, optional) receives the stream's figures.
    Witnesses that are torch GPU tensors are read where they lie; device_proof=True returns DeviceProof views of one GPU tensor.
    compact_wires: as in prove_streaming (the same proofs; `info` also receives "compact")."""
    _check_device_z64(device_compile, device_z64, device_b2a)
    dw = _wdev(wits_gf2, wits_z64, ctx, "prove_streaming_batch", batched=True)  # (refuses before a context is made)
    ctx = _ops_ctx(ops, ctx)
    ops, wire_counts, cinfo = _compacted(ops, wire_counts, ctx, compact_wires, prune, fold)
    if info is not None:
        _with_compact(info, cinfo)
    if dw is not None:  # (GPU tensors: [B][n] both, the batch from the descriptor)
        g0, z0, batch = wits_gf2, wits_z64, dw[1]
    else:
        g0 = np.asarray(wits_gf2, dtype=np.uint8)
        z0 = np.asarray(wits_z64, dtype=np.uint64)
        if g0.ndim == 2:  # (the batch is the first dimension of whichever witness array is 2-D: [] for the other domain)
            batch = g0.shape[0]
        elif z0.ndim == 2:
            batch = z0.shape[0]
        else:
            raise ValueError("wits_gf2 or wits_z64 must be [batch][n]")
    if _is_device_ops(ops) or dw is not None or device_proof:  # (begin / the feeds twice / finish)
        sp = StreamingBatchProver(wire_counts, batch, seeds, max_chunk_ops, ctx, device_compile, device_z64, device_b2a)
        try:
            sp.same_cuts()
            sp.feed(ops, g0, z0)
            sp.commit()
            sp.feed(ops, g0, z0)
            proofs = sp.finish(device=device_proof)
            if info is not None:
                info.update(sp.info)
            return proofs
        finally:
            sp.close()
    ops = program(ops) if len(ops) else np.zeros(0, OP_DTYPE)
    g = _eval_wits(g0, batch, np.uint8)
    z = _eval_wits(z0, batch, np.uint64)
    s = _batch_seeds(seeds, batch)
    outs = (C.c_void_p * batch)()
    lens = (C.c_size_t * batch)()
    si = _lib.StreamInfo()
    with _ctx_device_compile(ctx, device_compile, device_z64, device_b2a):
        _lib.check(_lib.lib().rv_prove_streaming_batch(ctx.handle, _ptr(ops), len(ops), int(wire_counts[0]), int(wire_counts[1]), batch, _ptr(g),
                                                       g.shape[1], _ptr(z), z.shape[1], _ptr(s), int(max_chunk_ops), outs, lens, C.byref(si)))
    if info is not None:
        info.update(_info(si))
    return [Proof(_owned=(C.c_void_p(outs[b]), int(lens[b]))) for b in range(batch)]


class StreamingBatchVerifier:
    """Proof::verify for several proofs of one statement over ONE streamed op list (rv_stream_verify_begin_batch).

        sv = StreamingBatchVerifier((z64_wires, gf2_wires), proofs)
        for ops in pieces: sv.feed(ops)
        oks = sv.finish()       # oks[b] == verify_streaming(all ops, ..., proofs[b]); a proof that cannot be parsed is False
    """

    def __init__(self, wire_counts: Tuple[int, int], proofs, max_chunk_ops: int = 0, ctx: Optional[Context] = None,
                 device_compile: bool = False, device_z64: bool = False, device_b2a: bool = False):
        _check_device_z64(device_compile, device_z64, device_b2a)
        self.ctx = ctx or Context.default()
        self.handle = C.c_void_p()
        self.batch = len(proofs)
        if self.batch < 1:
            raise ValueError("no proofs")
        dev = [_device_proof_bytes(p, ctx, "StreamingBatchVerifier") for p in proofs]
        if any(d is not None for d in dev):  # proofs in GPU memory, read in place: kept alive for the stream's life
            if any(d is None for d in dev):
                raise TypeError("StreamingBatchVerifier takes proofs that are all in GPU memory or all on the host")
            self._keep = [d[2] for d in dev]
            ptrs = (C.c_void_p * self.batch)(*[d[0] for d in dev])
            lens = (C.c_size_t * self.batch)(*[d[1] for d in dev])
            _lib.check(_lib.lib().rv_stream_verify_begin_batch_device(self.ctx.handle, int(wire_counts[0]), int(wire_counts[1]), self.batch, ptrs, lens,
                                                                      int(max_chunk_ops), C.byref(self.handle)))
            _set_device_compile(self.handle, device_compile, device_z64, device_b2a)
            return
        self._keep, ptrs, lens = _proof_array(proofs)  # (kept alive: the stream reads them until finish)
        _lib.check(_lib.lib().rv_stream_verify_begin_batch(self.ctx.handle, int(wire_counts[0]), int(wire_counts[1]), self.batch, ptrs, lens,
                                                           int(max_chunk_ops), C.byref(self.handle)))
        _set_device_compile(self.handle, device_compile, device_z64, device_b2a)

    feed = StreamingVerifier.feed

    def finish(self, strict: bool = True) -> "list[bool]":
        ok = (C.c_int * self.batch)()
        _lib.check(_lib.lib().rv_stream_verify_finish_batch(self.handle, 0 if strict else _lib.RV_VERIFY_REFERENCE_COMPAT, ok))
        return [bool(x) for x in ok]

    info = StreamingProver.info
    close = StreamingProver.close

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def verify_streaming_batch(ops, wire_counts: Tuple[int, int], proofs, strict: bool = True, max_chunk_ops: int = 0,
                           ctx: Optional[Context] = None, info: Optional[dict] = None, device_compile: bool = False, device_z64: bool = False, device_b2a: bool = False,
                           compact_wires: bool = False, prune: bool = False, fold: bool = False) -> "list[bool]":
    """rv_verify_streaming_batch: one pass over an op array in host memory for every proof -> one bool per proof.
    compact_wires: as in prove_streaming (the same answers; `info` also receives "compact")."""
    _check_device_z64(device_compile, device_z64, device_b2a)
    ctx = _ops_ctx(ops, ctx)
    n = len(proofs)
    if n == 0:
        return []
    ops, wire_counts, cinfo = _compacted(ops, wire_counts, ctx, compact_wires, prune, fold)
    if info is not None:
        _with_compact(info, cinfo)
    on_device = any(_device_proof_bytes(p, ctx, "verify_streaming_batch") is not None for p in proofs)
    if _is_device_ops(ops) or on_device:  # (begin / one feed / finish)
        sv = StreamingBatchVerifier(wire_counts, proofs, max_chunk_ops, ctx, device_compile, device_z64, device_b2a)
        try:
            sv.feed(ops)
            oks = sv.finish(strict)
            if info is not None:
                info.update(sv.info)
            return oks
        finally:
            sv.close()
    ops = program(ops) if len(ops) else np.zeros(0, OP_DTYPE)
    keep, ptrs, lens = _proof_array(proofs)
    ok = (C.c_int * n)()
    si = _lib.StreamInfo()
    with _ctx_device_compile(ctx, device_compile, device_z64, device_b2a):
        _lib.check(_lib.lib().rv_verify_streaming_batch(ctx.handle, _ptr(ops), len(ops), int(wire_counts[0]), int(wire_counts[1]), n, ptrs, lens,
                                                        0 if strict else _lib.RV_VERIFY_REFERENCE_COMPAT, int(max_chunk_ops), ok, C.byref(si)))
    del keep
    if info is not None:
        info.update(_info(si))
    return [bool(x) for x in ok]


def _eval_status(st: np.ndarray, gv, zv) -> Evaluation:
    n_failed = st[:, 0].astype(np.int64)
    return Evaluation(n_failed == 0, n_failed, st[:, 1].view(np.int64).copy(), gv, zv)


def _eval_wits(w, batch: int, dtype) -> np.ndarray:
    a = np.ascontiguousarray(np.asarray(w, dtype=dtype))
    if a.ndim == 1 and batch == 1:
        a = a.reshape(1, -1)
    if a.ndim == 1 and a.size == 0:
        a = np.zeros((batch, 0), dtype)
    if a.ndim != 2 or a.shape[0] != batch:
        raise ValueError(f"witnesses must be [batch={batch}][n] (1-D for batch 1)")
    return a


class StreamingEvaluator:
    """Cleartext evaluation of an op list fed in pieces, with bounded device memory (rv_eval_stream_*): what
    Circuit(all ops, keep_wires=True).evaluate_batch(..., values=True) computes, without compiling the whole list.

        se = StreamingEvaluator((z64_wires, gf2_wires), batch=B)
        for ops, w2, w64 in pieces: se.feed(ops, w2, w64)   # w2: [B][n] (1-D for B = 1), the elements these ops' Inputs consume
        r = se.finish(values=True)                            # the array-shaped Evaluation of Circuit.evaluate_batch

    Device memory is the wire store (wire counts x batch) plus one chunk of at most max_chunk_ops ops (0 = 2^18)."""

    def __init__(self, wire_counts: Tuple[int, int], batch: int = 1, max_chunk_ops: int = 0, ctx: Optional[Context] = None,
                 device_compile: bool = False, device_z64: bool = False, device_b2a: bool = False):
        _check_device_z64(device_compile, device_z64, device_b2a)
        self.ctx = ctx or Context.default()
        self.wire_counts = (int(wire_counts[0]), int(wire_counts[1]))
        self.batch = int(batch)
        self.handle = C.c_void_p()
        _lib.check(_lib.lib().rv_eval_stream_begin(self.ctx.handle, C.c_size_t(self.wire_counts[0]), C.c_size_t(self.wire_counts[1]),
                                                   C.c_size_t(self.batch), C.c_size_t(max_chunk_ops), C.byref(self.handle)))
        _set_device_compile(self.handle, device_compile, device_z64, device_b2a, "rv_eval_stream_set_compile_flags")

    def feed(self, ops, wits_gf2=(), wits_z64=()):
        dw = _wdev(wits_gf2, wits_z64, getattr(self, "ctx", None), "StreamingEvaluator.feed", batched=_rows_batched(wits_gf2, wits_z64, self.batch))
        if dw is not None:
            if dw[1] != self.batch:
                raise ValueError(f"witnesses must be [batch={self.batch}][n] (1-D for batch 1)")
            return _feed_wdev(self.handle, self.ctx, ops, dw, "rv_eval_stream_feed")
        g = _eval_wits(wits_gf2, self.batch, np.uint8)
        z = _eval_wits(wits_z64, self.batch, np.uint64)
        _feed(self.handle, self.ctx, ops, g, g.shape[1], z, z.shape[1], "rv_eval_stream_feed")

    def finish(self, values: bool = False) -> Evaluation:
        st = np.zeros((self.batch, 2), np.uint64)
        gv = np.zeros((self.batch, self.wire_counts[1]), np.uint8) if values else None
        zv = np.zeros((self.batch, self.wire_counts[0]), np.uint64) if values else None
        _lib.check(_lib.lib().rv_eval_stream_finish(self.handle, _ptr(gv), _ptr(zv), st.ctypes.data_as(C.c_void_p)))
        return _eval_status(st, gv, zv)

    @property
    def info(self) -> dict:
        si = _lib.EvalStreamInfo()
        _lib.check(_lib.lib().rv_eval_stream_get_info(self.handle, C.byref(si)))
        return {n: int(getattr(si, n)) for n, _ in si._fields_}

    def close(self):
        if self.handle:
            if self.ctx.handle:
                _lib.lib().rv_eval_stream_abort(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def evaluate_streaming(ops, wits_gf2, wits_z64, wire_counts: Tuple[int, int], max_chunk_ops: int = 0, values: bool = False,
                       ctx: Optional[Context] = None, info: Optional[dict] = None, device_compile: bool = False, device_z64: bool = False, device_b2a: bool = False,
                       compact_wires: bool = False, prune: bool = False, fold: bool = False) -> Evaluation:
    """rv_evaluate_streaming: one op array in host memory, evaluated chunk by chunk with bounded device memory.  wits_gf2 /
    wits_z64: [B][n] (1-D for one witness; the batch is len(wits_gf2)).  Returns the array-shaped Evaluation of
    Circuit.evaluate_batch; `info` (a dict, optional) receives the stream's figures.  compact_wires: the list is renumbered by
    liveness first; the statuses are the same, the wire values are those of the new indices under the new counts (an op's value
    lives at its renumbered `dst`: compact.compact_wires gives the renumbered list), and `info` also receives "compact"."""
    _check_device_z64(device_compile, device_z64, device_b2a)
    dims = [t.dim() for t in (wits_gf2, wits_z64) if hasattr(t, "data_ptr")]
    dw = _wdev(wits_gf2, wits_z64, ctx, "evaluate_streaming", batched=bool(dims) and max(dims) == 2)  # (refuses before a context is made)
    ctx = _ops_ctx(ops, ctx)
    ops, wire_counts, cinfo = _compacted(ops, wire_counts, ctx, compact_wires, prune, fold)
    if info is not None:
        _with_compact(info, cinfo)
    if dw is not None:
        g0, batch = wits_gf2, dw[1]
    else:
        g0 = np.asarray(wits_gf2, dtype=np.uint8)
        batch = g0.shape[0] if g0.ndim == 2 else 1
    if _is_device_ops(ops) or dw is not None:  # (begin / one feed / finish)
        se = StreamingEvaluator(wire_counts, batch, max_chunk_ops, ctx, device_compile, device_z64, device_b2a)
        try:
            se.feed(ops, g0, wits_z64)
            r = se.finish(values)
            if info is not None:
                info.update(se.info)
            return r
        finally:
            se.close()
    ops = program(ops) if len(ops) else np.zeros(0, OP_DTYPE)
    g = _eval_wits(g0, batch, np.uint8)
    z = _eval_wits(wits_z64, batch, np.uint64)
    wc = (int(wire_counts[0]), int(wire_counts[1]))
    st = np.zeros((batch, 2), np.uint64)
    gv = np.zeros((batch, wc[1]), np.uint8) if values else None
    zv = np.zeros((batch, wc[0]), np.uint64) if values else None
    si = _lib.EvalStreamInfo()
    with _ctx_device_compile(ctx, device_compile, device_z64, device_b2a):
        _lib.check(_lib.lib().rv_evaluate_streaming(ctx.handle, _ptr(ops), C.c_size_t(len(ops)), C.c_size_t(wc[0]), C.c_size_t(wc[1]),
                                                    C.c_size_t(batch), _ptr(g), C.c_size_t(g.shape[1]), _ptr(z), C.c_size_t(z.shape[1]),
                                                    C.c_size_t(max_chunk_ops), _ptr(gv), _ptr(zv), st.ctypes.data_as(C.c_void_p), C.byref(si)))
    if info is not None:
        info.update({k: int(getattr(si, k)) for k, _ in si._fields_})
    return _eval_status(st, gv, zv)


# ---- streams fed piece by piece from a source that is read again for every pass (a program file read in windows) ----
def _piece_inputs(ops, counts) -> Tuple[int, int]:
    """the Input ops of a piece per domain: what the piece's source counted -- (n_input_gf2, n_input_z64), or a piece dict of
    `program_file.DeviceReader.feed` -- or, where a piece comes with None, counted here"""
    if counts is not None:
        if isinstance(counts, dict):
            return int(counts["n_input_gf2"]), int(counts["n_input_z64"])
        return int(counts[0]), int(counts[1])
    if _is_device_ops(ops):  # (domain and opcode are a record's first two bytes)
        recs = ops.reshape(-1, OP_DTYPE.itemsize)
        inputs = recs[:, 1] == 0
        return int((inputs & (recs[:, 0] == 0)).sum()), int((inputs & (recs[:, 0] == 1)).sum())
    a = program(ops) if len(ops) else np.zeros(0, OP_DTYPE)
    inputs = a["opcode"] == 0
    return int(np.count_nonzero(inputs & (a["domain"] == 0))), int(np.count_nonzero(inputs & (a["domain"] == 1)))


def _is_wit_source(w) -> bool:
    """a GF(2) witness that is read as the pieces ask for it (`witness.DeviceWindows`): take(n) gives the next n bits as a GPU
    tensor, rewind() starts over"""
    return hasattr(w, "take") and hasattr(w, "rewind")


def _host_or_device_wit(w, dtype):
    return w if hasattr(w, "data_ptr") or _is_wit_source(w) else np.ascontiguousarray(np.asarray(w, dtype=dtype))


def _feed_pieces(feed, pieces, wit_gf2, wit_z64):
    """every piece of one pass to feed(ops, gf2 elements, z64 elements); the witnesses (the last axis) advance by the pieces' Input
    counts.  A GF(2) witness source is rewound first and gives each piece its bits with take."""
    used_g = used_z = 0
    source = _is_wit_source(wit_gf2)
    if source:
        wit_gf2.rewind()
    for ops, counts in (pieces() if callable(pieces) else pieces):
        if ops is None or len(ops) == 0:
            continue
        n_g, n_z = _piece_inputs(ops, counts)
        feed(ops, wit_gf2.take(n_g) if source else wit_gf2[..., used_g:used_g + n_g], wit_z64[..., used_z:used_z + n_z])
        used_g, used_z = used_g + n_g, used_z + n_z


def prove_streaming_pieces(pieces, wit_gf2, wit_z64, wire_counts: Tuple[int, int], seeds=None, max_chunk_ops: int = 0,
                           ctx: Optional[Context] = None, device_compile: bool = False, device_z64: bool = False, device_b2a: bool = False,
                           device_proof: bool = False, compact_wires: bool = False, prune: bool = False, fold: bool = False) -> "Tuple[Proof | DeviceProof, dict]":
    """`prove_streaming` for an op list that is never whole in memory: `pieces()` returns a fresh iterator of (ops, (n_input_gf2,
    n_input_z64)) for each of the two passes -- `program_file.iter_device` on a program file, say (its piece dicts serve as the
    counts).  ops: a host array or a torch GPU tensor of rv_op records; a host array may come with None, its Inputs are then counted
    here.  Both passes must yield the same pieces (rv_stream_same_cuts is set).  The proof is `prove_streaming`'s for the
    concatenated list; wire_counts are the whole list's (`program_file.scan_device`).  wit_gf2 may be a witness source that is read
    as the pieces ask for bits (`witness.DeviceWindows`: rewound at the start of each pass, take(n) per piece).  compact_wires: the pieces are renumbered by
    liveness in windows (`compact.compact_pieces`: the source is read for a scan pass first, twice with B2A ops), wire_counts are
    the source's and the stream begins with the new ones; the same proof, and info carries "compact".  prune: the ops no assertion
    depends on are dropped first, in windows (`prune.prune_pieces`: the pieces need `.backwards`, as `LinkPlan.pieces` and
    `prune.window_pieces` have it; the source is read for a scan pass and, backwards, for a mark pass), then compact_wires runs over
    the pruned pieces if asked for; the proof is the pruned list's (prover and verifier both pass prune=True), info carries "prune".
    fold=True is refused (ValueError): a window's unwritten index is not the list's; fold the whole list first (`fold.fold_ops`), or pass
    `fold.fold_pieces(pieces, wire_counts)[0]` as the pieces.
    -> (Proof or DeviceProof, stream info)"""
    if not callable(pieces):
        raise TypeError("prove_streaming_pieces reads the pieces twice: pass a callable that returns a fresh iterator")
    g, z = _host_or_device_wit(wit_gf2, np.uint8), _host_or_device_wit(wit_z64, np.uint64)
    pieces, wire_counts, cinfo, own = _compacted_pieces(pieces, wire_counts, ctx, compact_wires, prune, fold)
    sp = StreamingProver(wire_counts, seeds, max_chunk_ops, ctx, device_compile, device_z64, device_b2a)
    try:
        sp.same_cuts()
        _feed_pieces(sp.feed, pieces, g, z)
        sp.commit()
        _feed_pieces(sp.feed, pieces, g, z)
        return sp.finish(device=device_proof), _with_compact(sp.info, cinfo)
    finally:
        sp.close()
        if own is not None:
            own.close()


def verify_streaming_pieces(pieces, wire_counts: Tuple[int, int], proof, strict: bool = True, max_chunk_ops: int = 0,
                            ctx: Optional[Context] = None, device_compile: bool = False, device_z64: bool = False,
                            device_b2a: bool = False, compact_wires: bool = False, prune: bool = False, fold: bool = False) -> Tuple[bool, dict]:
    """`verify_streaming` for pieces as `prove_streaming_pieces` takes them (a callable or, the pass being one, an iterable; the
    counts are not looked at).  proof: bytes, a Proof, a bincode-form DeviceProof or a uint8 GPU tensor.  compact_wires: as in
    `prove_streaming_pieces` (a callable is needed then); prune: as there.  -> (ok, stream info)"""
    pieces, wire_counts, cinfo, own = _compacted_pieces(pieces, wire_counts, ctx, compact_wires, prune, fold)
    sv = StreamingVerifier(wire_counts, proof, max_chunk_ops, ctx, device_compile, device_z64, device_b2a)
    try:
        for ops, _ in (pieces() if callable(pieces) else pieces):
            if ops is not None and len(ops):
                sv.feed(ops)
        return sv.finish(strict), _with_compact(sv.info, cinfo)
    finally:
        sv.close()
        if own is not None:
            own.close()


def evaluate_streaming_pieces(pieces, wits_gf2, wits_z64, wire_counts: Tuple[int, int], max_chunk_ops: int = 0, values: bool = False,
                              ctx: Optional[Context] = None, info: Optional[dict] = None, device_compile: bool = False, device_z64: bool = False,
                              device_b2a: bool = False, compact_wires: bool = False, prune: bool = False, fold: bool = False) -> Evaluation:
    """`evaluate_streaming` for pieces as `prove_streaming_pieces` takes them, in one pass.  wits_gf2 / wits_z64: [B][n] (1-D for one
    witness), host arrays, torch GPU tensors or, for one GF(2) witness, a `witness.DeviceWindows`.  compact_wires: as in `prove_streaming_pieces` (wire values are those of the new
    indices); prune: as there.  -> the array-shaped Evaluation; `info` receives the stream's figures (and "compact", "prune")."""
    g, z = _host_or_device_wit(wits_gf2, np.uint8), _host_or_device_wit(wits_z64, np.uint64)
    pieces, wire_counts, cinfo, own = _compacted_pieces(pieces, wire_counts, ctx, compact_wires, prune, fold)
    batch = 1 if _is_wit_source(g) else g.shape[0] if g.ndim == 2 else 1
    se = StreamingEvaluator(wire_counts, batch, max_chunk_ops, ctx, device_compile, device_z64, device_b2a)
    try:
        _feed_pieces(se.feed, pieces, g, z)
        r = se.finish(values)
        if info is not None:
            info.update(_with_compact(se.info, cinfo))
        return r
    finally:
        se.close()
        if own is not None:
            own.close()
