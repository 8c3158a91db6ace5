"""Host-side mirror of the reference's `Proof` API for this path.

    reference (src/proof/mod.rs)                         here
    Proof::new(circuit, wit_gf2, wit_z64, (z64, gf2))    Proof.new(circuit, wit_gf2, wit_z64, (z64, gf2))
    proof.verify(circuit, (z64, gf2)) -> bool            proof.verify(circuit, (z64, gf2)) -> bool
    bincode::serialize(&proof)                           bytes(proof)     (byte-identical layout)
    bincode::deserialize(bytes)                          Proof(bytes)

`circuit` is an rv_op array (reverie_amd.ops.program) or an already compiled `Circuit`.
Everything runs through the C-ABI (include/reverie_amd.h) on the GPU; no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib
from .ops import OP_DTYPE, TOTAL_REPS, program


def _ptr(a: Optional[np.ndarray]):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


class Context:
    """One GPU (rv_ctx).  A default context on device 0 (or LOCAL_RANK) is created lazily."""

    _default = None

    def __init__(self, device: int = 0):
        self.handle = C.c_void_p()
        _lib.check(_lib.lib().rv_ctx_create(C.c_int(device), C.byref(self.handle)))
        self.device = device
        self.compile_flags = 0

    @classmethod
    def default(cls) -> "Context":
        if cls._default is None:
            import os

            cls._default = Context(int(os.environ.get("LOCAL_RANK", "0")))
        return cls._default

    def sync(self):
        _lib.check(_lib.lib().rv_ctx_sync(self.handle))

    def set_compile_flags(self, flags: int):
        """rv_ctx_set_compile_flags: 0 (default), RV_COMPILE_DEVICE or RV_COMPILE_DEVICE | RV_COMPILE_DEVICE_Z64 (Z64 and mixed programs
        and pieces on the GPU too; the bit alone is an error), the latter also with RV_COMPILE_DEVICE_B2A (programs and pieces with
        B2A ops too; an error without both other bits) -- the cold compiles of Proof.new_ops / verify_ops-style calls
        (rv_prove_ops, rv_verify_ops) then run on the GPU, and so do the piece compiles of the streams that begin afterwards
        (reverie_amd.stream).  Proof bytes and answers are unchanged."""
        _lib.check(_lib.lib().rv_ctx_set_compile_flags(self.handle, C.c_uint32(flags)))
        self.compile_flags = int(flags)

    def close(self):
        if self.handle:
            _lib.lib().rv_ctx_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _is_device_ops(ops) -> bool:
    """a torch tensor (torch stays an optional import: a caller who holds one has imported it)"""
    import sys

    torch = sys.modules.get("torch")
    return torch is not None and isinstance(ops, torch.Tensor)


def _device_ops(ops, ctx: "Optional[Context]", what: str) -> "Tuple[int, int, Context]":
    """(device pointer, n_ops, context) of an op list in GPU memory: a torch tensor on the context's device holding packed 24-byte
    rv_op records, as uint8 of shape [n, 24] (or [n * 24]) or int64 / uint64 of shape [n, 3]; contiguous.  Host memory is refused
    before any context is made (ctx None: the default one).  Waits for the tensor's device, so that the op list is complete before
    the library's stream reads it."""
    import torch

    if not isinstance(ops, torch.Tensor) or ops.device.type != "cuda":
        raise TypeError(f"{what} takes a torch tensor in GPU memory")
    if not ops.is_contiguous():
        raise ValueError("the op tensor must be contiguous")
    if ops.dtype == torch.uint8 and (ops.dim() == 1 and ops.numel() % OP_DTYPE.itemsize == 0 or ops.dim() == 2 and ops.shape[1] == OP_DTYPE.itemsize):
        n_ops = ops.numel() // OP_DTYPE.itemsize
    elif ops.dtype in (torch.int64, getattr(torch, "uint64", torch.int64)) and ops.dim() == 2 and ops.shape[1] == OP_DTYPE.itemsize // 8:
        n_ops = ops.shape[0]
    else:
        raise ValueError(f"op tensor must be uint8 [n, {OP_DTYPE.itemsize}] / [n * {OP_DTYPE.itemsize}] or int64 [n, 3], got "
                         f"{ops.dtype} {tuple(ops.shape)}")
    ctx = ctx or Context.default()
    if ops.device.index is not None and ops.device.index != ctx.device:
        raise ValueError(f"op tensor is on {ops.device}, the context on device {ctx.device}")
    torch.cuda.synchronize(ops.device)
    return ops.data_ptr(), n_ops, ctx


class Circuit:
    """A gate stream compiled (levelised) and resident in HBM (rv_circuit)."""

    def __init__(self, ops, wire_counts: Tuple[int, int], ctx: Optional[Context] = None, whole_prover: bool = False,
                 keep_wires: bool = False, device_compile: bool = False, device_z64: bool = False, device_b2a: bool = False,
                 device_keep_wires: bool = False):
        """whole_prover: the circuit will mostly serve whole proofs on one GPU (Proof.new / new_batch) -- the
        RV_COMPILE_WHOLE_PROVER hint of rv_circuit_compile_ex; any use of the circuit still gives identical bytes.
        keep_wires: RV_COMPILE_KEEP_WIRES -- the circuit keeps every wire's final value form, so that `evaluate` can return
        wire values (proofs stay byte-identical).
        device_compile: RV_COMPILE_DEVICE -- the ops are uploaded and compiled on the GPU (GF(2) programs, in the plain form or, with
        whole_prover, the lazy-sum form; anything the device path does not take is compiled on the host); the circuit is the same
        either way, and `compiled_on_device` tells which compiler made it.
        device_z64: RV_COMPILE_DEVICE_Z64, only with device_compile (ValueError otherwise) -- Z64 programs and programs that mix the
        two domains compile on the GPU too; B2A, a SizeHint that grows a wire count and keep_wires (without device_keep_wires) still go
        to the host compiler.
        device_b2a: RV_COMPILE_DEVICE_B2A, only with device_compile and device_z64 (ValueError otherwise) -- programs with B2A ops
        compile on the GPU too (plain form: when that is final, which of these deep programs only wide ones are; with whole_prover
        all of them).
        device_keep_wires: RV_COMPILE_DEVICE_KEEP_WIRES, only with keep_wires and device_compile (ValueError otherwise) -- keep_wires
        no longer sends the program to the host compiler: the device compiler builds the wires' final forms too, in every scope the
        other device keywords open, and `evaluate` returns the same values."""
        if device_keep_wires and not (keep_wires and device_compile):
            raise ValueError("device_keep_wires=True needs " + " and ".join(
                k + "=True" for k, v in (("keep_wires", keep_wires), ("device_compile", device_compile)) if not v))
        if device_z64 and not device_compile:
            raise ValueError("device_z64=True needs device_compile=True")
        if device_b2a and not (device_compile and device_z64):
            raise ValueError("device_b2a=True needs device_compile=True and device_z64=True")
        self.ctx = ctx or Context.default()
        self.ops = program(ops) if len(ops) else np.zeros(0, OP_DTYPE)
        self.wire_counts = (int(wire_counts[0]), int(wire_counts[1]))  # (z64, gf2), proof/mod.rs:125
        self.keep_wires = bool(keep_wires)
        self.handle = C.c_void_p()
        flags = (_lib.RV_COMPILE_WHOLE_PROVER if whole_prover else 0) | (_lib.RV_COMPILE_KEEP_WIRES if keep_wires else 0) | \
            (_lib.RV_COMPILE_DEVICE if device_compile else 0) | (_lib.RV_COMPILE_DEVICE_Z64 if device_z64 else 0) | \
            (_lib.RV_COMPILE_DEVICE_B2A if device_b2a else 0) | (_lib.RV_COMPILE_DEVICE_KEEP_WIRES if device_keep_wires else 0)
        _lib.check(_lib.lib().rv_circuit_compile_ex(self.ctx.handle, _ptr(self.ops), C.c_size_t(len(self.ops)),
                                                    C.c_size_t(self.wire_counts[0]), C.c_size_t(self.wire_counts[1]),
                                                    C.c_uint32(flags), C.byref(self.handle)))

    @classmethod
    def from_device_ops(cls, ops, wire_counts: Tuple[int, int], ctx: Optional[Context] = None, whole_prover: bool = False,
                        keep_wires: bool = False, device_z64: bool = False, device_b2a: bool = False,
                        device_keep_wires: bool = False) -> "Circuit":
        """rv_circuit_compile_device: compile an op list that already sits in GPU memory -- a torch tensor on the context's
        device holding packed 24-byte rv_op records, as uint8 of shape [n, 24] (or [n * 24]) or int64 / uint64 of shape [n, 3];
        contiguous.  The tensor is not copied to the host unless the device path hands the program to the host compiler; the
        caller keeps it.  The circuit is the one Circuit(host ops, device_compile=True) compiles, with whole_prover the lazy-sum
        form (also built on the device).  device_z64: RV_COMPILE_DEVICE_Z64 -- Z64 and mixed programs are compiled where they are too
        (the call itself is the device compile the bit needs).  device_b2a: RV_COMPILE_DEVICE_B2A, only with device_z64 (ValueError
        otherwise) -- programs with B2A ops too.  device_keep_wires: RV_COMPILE_DEVICE_KEEP_WIRES, only with keep_wires (ValueError
        otherwise; the call itself is the device compile the bit needs) -- a keep_wires program is compiled where it is as well,
        instead of being copied to the host."""
        if device_keep_wires and not keep_wires:
            raise ValueError("device_keep_wires=True needs keep_wires=True")
        if device_b2a and not device_z64:
            raise ValueError("device_b2a=True needs device_z64=True")
        d_ops, n_ops, ctx = _device_ops(ops, ctx, "from_device_ops")
        self = cls.__new__(cls)
        self.ctx = ctx
        self.ops = None  # (on the device only)
        self.wire_counts = (int(wire_counts[0]), int(wire_counts[1]))
        self.keep_wires = bool(keep_wires)
        self.handle = C.c_void_p()
        flags = (_lib.RV_COMPILE_WHOLE_PROVER if whole_prover else 0) | (_lib.RV_COMPILE_KEEP_WIRES if keep_wires else 0) | \
            (_lib.RV_COMPILE_DEVICE_Z64 if device_z64 else 0) | (_lib.RV_COMPILE_DEVICE_B2A if device_b2a else 0) | \
            (_lib.RV_COMPILE_DEVICE_KEEP_WIRES if device_keep_wires else 0)
        _lib.check(_lib.lib().rv_circuit_compile_device(self.ctx.handle, C.c_void_p(d_ops), C.c_size_t(n_ops),
                                                        C.c_size_t(self.wire_counts[0]), C.c_size_t(self.wire_counts[1]),
                                                        C.c_uint32(flags), C.byref(self.handle)))
        return self

    @property
    def info(self) -> dict:
        ci = _lib.CircuitInfo()
        _lib.check(_lib.lib().rv_circuit_get_info(self.handle, C.byref(ci)))
        d = {n: int(getattr(ci, n)) for n, _ in ci._fields_}
        esb = C.c_uint64()
        _lib.check(_lib.lib().rv_circuit_early_staging_bytes(self.handle, C.byref(esb)))
        d["early_staging_bytes"] = int(esb.value)
        return d

    @property
    def compiled_on_device(self) -> bool:
        """rv_circuit_compiled_on_device: True when the device compiler made this circuit, False when the host compiler did (no
        device_compile, or a program the device path handed back)."""
        on = C.c_int()
        _lib.check(_lib.lib().rv_circuit_compiled_on_device(self.handle, C.byref(on)))
        return bool(on.value)

    def evaluate(self, wit_gf2, wit_z64=()) -> "Evaluation":
        """Cleartext evaluation on the GPU (rv_evaluate): `ok`, `n_failed`, `first_failed_op` (op-list index of the first
        failing AssertZero, None if all hold) and, for a circuit compiled with keep_wires, the wires' final values `gf2`
        (uint8, one per GF(2) wire) and `z64` (uint64).  A failing assertion is a result, not an error."""
        g, z = _witness(wit_gf2, wit_z64)
        st = _lib.EvalStatus()
        gv = np.zeros(self.wire_counts[1], np.uint8) if self.keep_wires else None
        zv = np.zeros(self.wire_counts[0], np.uint64) if self.keep_wires else None
        _lib.check(_lib.lib().rv_evaluate(self.ctx.handle, self.handle, _ptr(g), C.c_size_t(len(g)), _ptr(z), C.c_size_t(len(z)),
                                          _ptr(gv) if gv is not None else None, _ptr(zv) if zv is not None else None, C.byref(st)))
        first = None if st.first_failed_op == 0xFFFFFFFFFFFFFFFF else int(st.first_failed_op)
        return Evaluation(st.n_failed == 0, int(st.n_failed), first, gv, zv)

    def evaluate_batch(self, wits_gf2, wits_z64=None, values: bool = False) -> "Evaluation":
        """rv_evaluate_batch: `len(wits_gf2)` witnesses ([B][n] bits; wits_z64 [B][m] words or None) in one pass.  Returns
        arrays: `ok` (bool [B]), `n_failed` ([B]), `first_failed_op` ([B] int64, -1 where every assertion holds) and, with
        values=True (needs keep_wires), `gf2` ([B][gf2_wires] uint8) and `z64` ([B][z64_wires] uint64).  Witness b's results
        equal evaluate(wits_gf2[b], wits_z64[b])."""
        g = np.ascontiguousarray(np.asarray(wits_gf2, dtype=np.uint8))
        if g.ndim != 2:
            raise ValueError("wits_gf2 must be [batch][n_bits]")
        batch = g.shape[0]
        z = np.ascontiguousarray(np.asarray(wits_z64 if wits_z64 is not None else np.zeros((batch, 0)), dtype=np.uint64))
        if z.ndim != 2 or z.shape[0] != batch:
            raise ValueError("wits_z64 must be [batch][n_words]")
        st = np.zeros((max(batch, 1), 2), np.uint64)
        gv = np.zeros((batch, self.wire_counts[1]), np.uint8) if values else None
        zv = np.zeros((batch, self.wire_counts[0]), np.uint64) if values else None
        if batch:
            _lib.check(_lib.lib().rv_evaluate_batch(self.ctx.handle, self.handle, C.c_size_t(batch), _ptr(g), C.c_size_t(g.shape[1]), _ptr(z),
                                                    C.c_size_t(z.shape[1]), _ptr(gv) if values else None, _ptr(zv) if values else None,
                                                    st.ctypes.data_as(C.c_void_p)))
        st = st[:batch]
        n_failed = st[:, 0].astype(np.int64)
        return Evaluation(n_failed == 0, n_failed, st[:, 1].view(np.int64).copy(), gv, zv)

    def evaluate_batch_device(self, wits_gf2, wits_z64=None, gf2_wires=None, z64_wires=None) -> "DeviceEvaluation":
        """rv_evaluate_batch_device: evaluate_batch on witnesses that lie in GPU memory, with the results left there.  wits_gf2 /
        wits_z64: torch GPU tensors on the circuit's device in the forms `_device_witness` takes ([B][n] uint8 or bool, [B][m] int64 or
        uint64; a row stride is allowed); anything else raises TypeError.  gf2_wires / z64_wires: None = no values of that domain,
        ... (Ellipsis) = every wire in order, or a sequence of wire indices (unsorted, repeats allowed; values need keep_wires).
        -> DeviceEvaluation; column i of its `gf2` / `z64` equals column wires[i] of evaluate_batch(values=True).  No witness and no
        result crosses to the host."""
        import torch

        dw = _device_witness(wits_gf2, wits_z64, self.ctx, "evaluate_batch_device", batched=True)
        if dw is None:
            raise TypeError("evaluate_batch_device takes torch tensors in GPU memory")
        w, batch, _keep, _ = dw
        dev = f"cuda:{self.ctx.device}"

        def selection(wires, n_wires, dtype):
            # -> (host index array or None, its ctypes pointer, n_sel, values tensor or None)
            if wires is None:
                return None, None, 0, None
            if wires is Ellipsis:
                return None, None, 0, torch.empty((batch, n_wires), dtype=dtype, device=dev)
            idx = np.ascontiguousarray(np.asarray(wires, dtype=np.int64).reshape(-1))
            if idx.size and (idx.min() < 0 or idx.max() > 0xFFFFFFFF):
                raise ValueError("wire indices are unsigned 32-bit numbers")
            sel = np.zeros(max(idx.size, 1), np.uint32)  # (never NULL: an empty list asks for no wire, not for every wire)
            sel[:idx.size] = idx
            return sel, sel.ctypes.data_as(C.c_void_p), idx.size, torch.empty((batch, idx.size), dtype=dtype, device=dev)

        s2, p2, n2, gv = selection(gf2_wires, self.wire_counts[1], torch.uint8)
        s64, p64, n64, zv = selection(z64_wires, self.wire_counts[0], torch.int64)
        status = torch.empty((batch, 2), dtype=torch.int64, device=dev)
        _lib.check(_lib.lib().rv_evaluate_batch_device(
            self.ctx.handle, self.handle, C.c_size_t(batch), C.byref(w), p2, C.c_size_t(n2), p64, C.c_size_t(n64),
            C.c_void_p(gv.data_ptr()) if gv is not None else None, C.c_void_p(zv.data_ptr()) if zv is not None else None,
            C.c_void_p(status.data_ptr())))
        return DeviceEvaluation(status, gv, zv)

    def record_sizes(self) -> Tuple[int, int]:
        """bytes of one OpenOnline record in the gf2 / z64 section of a proof of this circuit"""
        a, b = C.c_size_t(), C.c_size_t()
        _lib.check(_lib.lib().rv_circuit_record_sizes(self.handle, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def close(self):
        if self.handle:
            if self.ctx.handle:  # a circuit lives in its context's arena: once that is gone there is nothing left to free
                _lib.lib().rv_circuit_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Evaluation:
    """What Circuit.evaluate / evaluate_batch return (scalars for one witness, arrays for a batch)."""

    def __init__(self, ok, n_failed, first_failed_op, gf2=None, z64=None):
        self.ok, self.n_failed, self.first_failed_op, self.gf2, self.z64 = ok, n_failed, first_failed_op, gf2, z64

    def __repr__(self):
        return f"Evaluation(ok={self.ok!r}, n_failed={self.n_failed!r}, first_failed_op={self.first_failed_op!r})"


class DeviceEvaluation:
    """What Circuit.evaluate_batch_device returns: torch tensors on the circuit's device.  `status` is int64 [B][2] (the
    rv_eval_status records); `n_failed`, `first_failed_op` (-1 where every assertion holds) and `ok` are views of it resp. computed
    from it on the device; `gf2` is uint8 [B][n_sel] and `z64` int64 [B][n_sel] (the words' bits), None where no values were asked."""

    def __init__(self, status, gf2=None, z64=None):
        self.status, self.gf2, self.z64 = status, gf2, z64

    @property
    def n_failed(self):
        return self.status[:, 0]

    @property
    def first_failed_op(self):
        return self.status[:, 1]

    @property
    def ok(self):
        return self.status[:, 0] == 0

    def __repr__(self):
        return f"DeviceEvaluation(batch={self.status.shape[0]}, device={self.status.device})"


def evaluate_composite_program(ops, wit_gf2, wit_z64=(), wire_counts=None, ctx: Optional[Context] = None):
    """mcircuit::evaluate_composite_program, which the reference re-exports (src/lib.rs:6) and its CLI's `oneshot` calls
    (src/main.rs:115-132): the op list evaluated in the clear on the witness -> (gf2, z64) wire vectors (uint8 / uint64) at the
    end of the program.  Raises ValueError naming the op index of the first AssertZero that does not hold.  The crate's exact
    signature and return type cannot be checked here (it is not vendored); this is the evaluation it names, on the
    GPU (rv_evaluate).  wire_counts (z64, gf2) defaults to largest_wires(ops)."""
    from .ops import largest_wires

    prog = program(ops) if len(ops) else np.zeros(0, OP_DTYPE)
    wc = tuple(wire_counts) if wire_counts is not None else largest_wires(prog)
    r = Circuit(prog, wc, ctx, keep_wires=True).evaluate(wit_gf2, wit_z64)
    if not r.ok:
        raise ValueError(f"AssertZero at op {r.first_failed_op} does not hold ({r.n_failed} failing assertions)")
    return r.gf2, r.z64


def _as_circuit(circuit, wire_counts, ctx=None, whole_prover=False) -> Circuit:
    if isinstance(circuit, Circuit):
        if wire_counts is not None and tuple(wire_counts) != circuit.wire_counts:
            raise ValueError("wire_counts differ from the compiled circuit's")
        return circuit
    return Circuit(circuit, wire_counts, ctx, whole_prover=whole_prover)


def _witness(wit_gf2, wit_z64):
    g = np.ascontiguousarray(np.asarray(wit_gf2, dtype=np.uint8))
    z = np.ascontiguousarray(np.asarray(wit_z64, dtype=np.uint64))
    return g, z


def _device_witness(wit_gf2, wit_z64, ctx: "Optional[Context]", what: str, batched: bool):
    """The witnesses of a call as an rv_dev_witness when they lie in GPU memory: -> (descriptor, batch, the tensors (kept alive by
    the caller for the call), context), or None when neither is a torch GPU tensor (the call then goes the host way, as ever).
    Taken: uint8 or bool tensors [n] (batched: [B][n]) for GF(2), int64 or uint64 tensors [m] ([B][m]) for Z64, on the context's
    device, the last dimension contiguous; a row stride is allowed.  The other witness may be absent (None or empty); one witness in
    GPU memory and the other on the host is a TypeError.  Refuses before any context is made (ctx None: the default one), and waits
    for the tensors' device, so that the witnesses are complete before the library's stream reads them."""
    import sys

    torch = sys.modules.get("torch")

    def on_gpu(t):
        return torch is not None and isinstance(t, torch.Tensor) and t.device.type == "cuda"

    g_dev, z_dev = on_gpu(wit_gf2), on_gpu(wit_z64)
    if not g_dev and not z_dev:
        return None
    for t, here in ((wit_gf2, g_dev), (wit_z64, z_dev)):
        if not here and t is not None and np.size(t):
            raise TypeError(f"{what}: one witness is in GPU memory and the other on the host")
    dims = 2 if batched else 1
    w = _lib.DevWitness()
    batch = None
    device = None
    for name, t, dtypes in (("gf2", wit_gf2 if g_dev else None, (torch.uint8, torch.bool)),
                            ("z64", wit_z64 if z_dev else None, (torch.int64, getattr(torch, "uint64", torch.int64)))):
        if t is None:
            continue
        if t.dtype not in dtypes or t.dim() != dims or (t.shape[-1] > 1 and t.stride(-1) != 1) or \
                (batched and t.shape[0] > 1 and t.stride(0) < t.shape[1]):
            raise ValueError(f"{what}: the {name} witness must be {' or '.join(str(d) for d in dtypes)} "
                             f"{'[batch][n]' if batched else '[n]'} with a contiguous last dimension, got {t.dtype} {tuple(t.shape)} "
                             f"strides {tuple(t.stride())}")
        if batched:
            if batch is not None and t.shape[0] != batch:
                raise ValueError(f"{what}: the witnesses' batch sizes differ")
            batch = t.shape[0]
        if device is not None and t.device != device:
            raise ValueError(f"{what}: the witnesses are on different devices")
        device = t.device
        setattr(w, name, t.data_ptr() if t.numel() else None)
        setattr(w, "n_" + name, t.shape[-1])
        setattr(w, "stride_" + name, t.stride(0) if batched and t.shape[0] > 1 else t.shape[-1])
    ctx = ctx or Context.default()
    if device.index is not None and device.index != ctx.device:
        raise ValueError(f"the witness is on {device}, the context on device {ctx.device}")
    torch.cuda.synchronize(device)
    return w, (batch if batched else 1), (wit_gf2, wit_z64), ctx


class Proof:
    """bincode(Proof) bytes.  A proof that came out of rv_prove stays in the library's (page-locked) buffer
    until it is dropped — `bytes(proof)` copies it out, `verify` reads it in place."""

    def __init__(self, data: bytes = b"", _owned=None):
        self._bytes = None if _owned is not None else bytes(data)
        self._ptr, self._len = _owned if _owned is not None else (None, len(self._bytes))
        if _owned is not None:
            import weakref

            weakref.finalize(self, _lib.lib().rv_free, self._ptr)

    @property
    def data(self) -> bytes:
        if self._bytes is None:
            self._bytes = C.string_at(self._ptr, self._len)
        return self._bytes

    def __bytes__(self):
        return self.data

    def __len__(self):
        return self._len

    @property
    def comm(self) -> bytes:
        return C.string_at(self._ptr, 32) if self._bytes is None else self._bytes[:32]

    def _buffer(self):
        """(pointer, length) of the proof bytes without copying them"""
        if self._ptr is not None:
            return self._ptr, self._len
        return C.cast(C.c_char_p(self._bytes), C.c_void_p), self._len

    @staticmethod
    def new(circuit, wit_gf2: Sequence[int], wit_z64: Sequence[int], wire_counts: Optional[Tuple[int, int]] = None,
            seeds: Union[None, bytes, np.ndarray] = None, ctx: Optional[Context] = None) -> "Proof":
        """Proof::new.  `seeds` (256x16 bytes) injects the per-repetition seeds the reference
        draws from OsRng; None draws them from the OS.  Witnesses that are torch GPU tensors (`_device_witness`) are read where
        they lie (rv_prove_wdev; a raw op list is compiled first): the proof is the one their host copies give."""
        dw = _device_witness(wit_gf2, wit_z64, circuit.ctx if isinstance(circuit, Circuit) else ctx, "Proof.new", batched=False)
        g, z = _witness(wit_gf2, wit_z64) if dw is None else (None, None)
        s = None
        if seeds is not None:
            s = np.ascontiguousarray(np.frombuffer(bytes(seeds), np.uint8) if isinstance(seeds, (bytes, bytearray))
                                     else np.asarray(seeds, dtype=np.uint8)).reshape(TOTAL_REPS, 16)
        out = C.c_void_p()
        n = C.c_size_t()
        if dw is not None:
            c = _as_circuit(circuit, wire_counts, dw[3])
            _lib.check(_lib.lib().rv_prove_wdev(c.ctx.handle, c.handle, C.byref(dw[0]), _ptr(s), C.byref(out), C.byref(n)))
        elif isinstance(circuit, Circuit):
            c = _as_circuit(circuit, wire_counts, ctx)
            _lib.check(_lib.lib().rv_prove(c.ctx.handle, c.handle, _ptr(g), C.c_size_t(len(g)), _ptr(z), C.c_size_t(len(z)),
                                           _ptr(s), C.byref(out), C.byref(n)))
        else:
            # the reference's own call shape (proof/mod.rs:119-125): the raw op list, compiled for this one proof
            ops = program(circuit) if len(circuit) else np.zeros(0, OP_DTYPE)
            cx = ctx or Context.default()
            _lib.check(_lib.lib().rv_prove_ops(cx.handle, ops.ctypes.data_as(C.c_void_p), C.c_size_t(len(ops)), _ptr(g), C.c_size_t(len(g)),
                                               _ptr(z), C.c_size_t(len(z)), C.c_size_t(int(wire_counts[0])), C.c_size_t(int(wire_counts[1])),
                                               _ptr(s), C.byref(out), C.byref(n)))
        return Proof(_owned=(C.c_void_p(out.value), n.value))

    @staticmethod
    def new_batch(circuit, wits_gf2, wits_z64=None, wire_counts: Optional[Tuple[int, int]] = None, seeds=None,
                  ctx: Optional[Context] = None) -> "list[Proof]":
        """`len(wits_gf2)` proofs of one circuit in one pass (rv_prove_batch): every dependency level is launched
        once for the whole batch.  wits_gf2: [B][n] bits; wits_z64: [B][m] words or None; seeds: [B][256][16] bytes or
        None (OS randomness).  Each proof equals Proof.new(circuit, wits_gf2[b], wits_z64[b], seeds=seeds[b]).  Witnesses that are
        torch GPU tensors (`_device_witness`; rows may be strided) are read where they lie (rv_prove_batch_wdev)."""
        dw = _device_witness(wits_gf2, wits_z64, circuit.ctx if isinstance(circuit, Circuit) else ctx, "Proof.new_batch", batched=True)
        c = _as_circuit(circuit, wire_counts, ctx if dw is None else dw[3], whole_prover=True)
        if dw is None:
            g = np.ascontiguousarray(np.asarray(wits_gf2, dtype=np.uint8))
            if g.ndim != 2:
                raise ValueError("wits_gf2 must be [batch][n_bits]")
            batch = g.shape[0]
            z = np.ascontiguousarray(np.asarray(wits_z64 if wits_z64 is not None else np.zeros((batch, 0)), dtype=np.uint64))
            if z.ndim != 2 or z.shape[0] != batch:
                raise ValueError("wits_z64 must be [batch][n_words]")
        else:
            batch = dw[1]
        s = None
        if seeds is not None:
            s = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint8)).reshape(batch, TOTAL_REPS, 16)
        outs = (C.c_void_p * batch)()
        lens = (C.c_size_t * batch)()
        if dw is not None:
            _lib.check(_lib.lib().rv_prove_batch_wdev(c.ctx.handle, c.handle, C.c_size_t(batch), C.byref(dw[0]), _ptr(s), outs, lens))
        else:
            _lib.check(_lib.lib().rv_prove_batch(c.ctx.handle, c.handle, C.c_size_t(batch), _ptr(g), C.c_size_t(g.shape[1]), _ptr(z),
                                                 C.c_size_t(z.shape[1]), _ptr(s), outs, lens))
        return [Proof(_owned=(C.c_void_p(outs[b]), int(lens[b]))) for b in range(batch)]

    def verify(self, circuit, wire_counts: Optional[Tuple[int, int]] = None, ctx: Optional[Context] = None,
               strict: bool = True) -> bool:
        """Proof::verify (/root/reference/src/proof/mod.rs:224-307), strict by default: the opened repetitions'
        AssertZero gates must hold and the records' `omit` must match the challenge -- both of which the reference
        leaves unchecked, so that it accepts proofs of false statements.  strict=False is
        RV_VERIFY_REFERENCE_COMPAT: exactly the reference's answer (compatibility tests only)."""
        ok = C.c_int()
        buf, n = self._buffer()
        flags = 0 if strict else _lib.RV_VERIFY_REFERENCE_COMPAT
        if isinstance(circuit, Circuit):
            c = _as_circuit(circuit, wire_counts, ctx)
            _lib.check(_lib.lib().rv_verify_ex(c.ctx.handle, c.handle, buf, C.c_size_t(n), C.c_uint32(flags), C.byref(ok)))
        else:
            ops = program(circuit) if len(circuit) else np.zeros(0, OP_DTYPE)
            cx = ctx or Context.default()
            _lib.check(_lib.lib().rv_verify_ops(cx.handle, ops.ctypes.data_as(C.c_void_p), C.c_size_t(len(ops)), C.c_size_t(int(wire_counts[0])),
                                                C.c_size_t(int(wire_counts[1])), buf, C.c_size_t(n), C.c_uint32(flags), C.byref(ok)))
        return bool(ok.value)


def _device_bytes(t, ctx: "Optional[Context]", what: str) -> "Tuple[int, int, Context]":
    """(device pointer, length, context) of proof bytes in GPU memory: a contiguous one-dimensional torch uint8 tensor on the
    context's device.  Host tensors and tensors of another device are refused before any library call (ctx None: the default
    context).  Waits for the tensor's device, so that the bytes are complete before the library's stream reads them."""
    import torch

    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise TypeError(f"{what} takes a torch tensor in GPU memory")
    if t.dtype != torch.uint8 or t.dim() != 1 or not t.is_contiguous():
        raise ValueError(f"{what} takes a contiguous one-dimensional uint8 tensor, got {t.dtype} {tuple(t.shape)}")
    ctx = ctx or Context.default()
    if t.device.index is not None and t.device.index != ctx.device:
        raise ValueError(f"the tensor is on {t.device}, the context on device {ctx.device}")
    torch.cuda.synchronize(t.device)
    return t.data_ptr(), t.numel(), ctx


class DeviceProof:
    """A proof that lies in GPU memory, verified where it is (rv_verify_device / rv_verify_sections_device): either

        DeviceProof(tensor)                            bincode(Proof) bytes in a torch uint8 GPU tensor
        DeviceProof(sections=t, lens=[..], comm=b)     what rv_prove_device left: [gf2 online | gf2 preprocessing | z64 online |
                                                       z64 preprocessing] in `t`, the four lengths, the commitment (host bytes)

    The tensor stays the caller's; it must start on a 16-byte boundary (a fresh torch allocation does).  `verify` answers what
    `Proof.verify` answers on the same bytes; no proof byte is copied to the host unless the bytes are not a well-framed proof."""

    def __init__(self, tensor=None, *, sections=None, lens=None, comm=None, ctx: Optional[Context] = None):
        if (tensor is None) == (sections is None):
            raise ValueError("DeviceProof takes a tensor of proof bytes, or sections with lens and comm")
        if sections is not None:
            if lens is None or comm is None or len(lens) != 4 or len(bytes(comm)) != 32:
                raise ValueError("sections come with their four lengths and the 32-byte commitment")
            self.lens = [int(x) for x in lens]
            self._comm = bytes(comm)
            self._ptr, n, self.ctx = _device_bytes(sections, ctx, "DeviceProof")
            if sum(self.lens) > n:
                raise ValueError(f"the sections' lengths add up to {sum(self.lens)} bytes, the tensor has {n}")
        else:
            self.lens = None
            self._comm = None
            self._ptr, self._len, self.ctx = _device_bytes(tensor, ctx, "DeviceProof")
        self.tensor = tensor if tensor is not None else sections  # (keeps the memory alive)

    @staticmethod
    def new(circuit: "Circuit", wit_gf2: Sequence[int], wit_z64: Sequence[int], seeds: Union[None, bytes, np.ndarray] = None,
            ctx: Optional[Context] = None) -> "DeviceProof":
        """rv_prove_device: Proof::new with the openings left in GPU memory (the sections form).  `seeds` (256 x 16 bytes) as
        Proof.new; None draws them from the OS (the entry point takes no NULL).  Witnesses that are torch GPU tensors
        (`_device_witness`) are read where they lie (rv_prove_device_wdev)."""
        import os

        import torch

        if not isinstance(circuit, Circuit):
            raise TypeError("DeviceProof.new takes a compiled Circuit")
        if ctx is not None and ctx is not circuit.ctx:
            raise ValueError("the circuit was compiled in another context")
        dw = _device_witness(wit_gf2, wit_z64, circuit.ctx, "DeviceProof.new", batched=False)
        g, z = _witness(wit_gf2, wit_z64) if dw is None else (None, None)
        raw = os.urandom(TOTAL_REPS * 16) if seeds is None else (bytes(seeds) if isinstance(seeds, (bytes, bytearray)) else None)
        s = np.ascontiguousarray(np.frombuffer(raw, np.uint8) if raw is not None else np.asarray(seeds, dtype=np.uint8)).reshape(TOTAL_REPS, 16)
        sz2, sz64 = circuit.record_sizes()
        out = torch.empty(40 * (sz2 + sz64) + 2 * (TOTAL_REPS - 40) * 48, dtype=torch.uint8, device=f"cuda:{circuit.ctx.device}")
        lens = (C.c_size_t * 4)()
        comm = np.zeros(32, np.uint8)
        omit = np.zeros(TOTAL_REPS, np.uint8)
        if dw is not None:
            _lib.check(_lib.lib().rv_prove_device_wdev(circuit.ctx.handle, circuit.handle, C.byref(dw[0]), _ptr(s), C.c_void_p(out.data_ptr()),
                                                       _ptr(comm), _ptr(omit), lens))
        else:
            _lib.check(_lib.lib().rv_prove_device(circuit.ctx.handle, circuit.handle, _ptr(g), C.c_size_t(len(g)), _ptr(z), C.c_size_t(len(z)),
                                                  _ptr(s), C.c_void_p(out.data_ptr()), _ptr(comm), _ptr(omit), lens))
        return DeviceProof(sections=out, lens=[int(x) for x in lens], comm=comm.tobytes(), ctx=circuit.ctx)

    @property
    def comm(self) -> bytes:
        if self._comm is None:
            self._comm = bytes(self.tensor[:32].cpu().numpy().tobytes())
        return self._comm

    def verify(self, circuit: "Circuit", strict: bool = True) -> bool:
        """Proof.verify(circuit, strict=strict) on these bytes, read in GPU memory"""
        if not isinstance(circuit, Circuit):
            raise TypeError("DeviceProof.verify takes a compiled Circuit")
        if circuit.ctx.device != self.ctx.device:
            raise ValueError(f"the proof is on device {self.ctx.device}, the circuit's context on device {circuit.ctx.device}")
        ok = C.c_int()
        flags = 0 if strict else _lib.RV_VERIFY_REFERENCE_COMPAT
        if self.lens is None:
            _lib.check(_lib.lib().rv_verify_device(circuit.ctx.handle, circuit.handle, C.c_void_p(self._ptr), C.c_size_t(self._len),
                                                   C.c_uint32(flags), C.byref(ok)))
        else:
            comm = np.frombuffer(self._comm, np.uint8)
            _lib.check(_lib.lib().rv_verify_sections_device(circuit.ctx.handle, circuit.handle, _ptr(comm), C.c_void_p(self._ptr),
                                                            (C.c_size_t * 4)(*self.lens), C.c_uint32(flags), C.byref(ok)))
        return bool(ok.value)

    def to_proof(self) -> "Proof":
        """the bytes as a host `Proof` (one copy down; sections are framed by rv_assemble_proof)"""
        host = self.tensor.cpu().numpy()
        if self.lens is None:
            return Proof(host.tobytes())
        parts = _lib.ShardParts()
        at = 0
        for name, n in zip(("gf2_online", "gf2_pre", "z64_online", "z64_pre"), self.lens):
            setattr(parts, name, host.ctypes.data + at)
            setattr(parts, name + "_len", n)
            at += n
        parts.n_online, parts.n_pre = 40, TOTAL_REPS - 40
        comm = np.frombuffer(self._comm, np.uint8)
        out = C.c_void_p()
        n = C.c_size_t()
        _lib.check(_lib.lib().rv_assemble_proof(_ptr(comm), C.byref(parts), C.c_size_t(1), C.byref(out), C.byref(n)))
        return Proof(_owned=(C.c_void_p(out.value), n.value))


def verify_batch(circuit, proofs, wire_counts: Optional[Tuple[int, int]] = None, ctx: Optional[Context] = None,
                 strict: bool = True) -> "list[bool]":
    """rv_verify_batch: Proof.verify for many proofs of one circuit in one pass (`proofs`: Proof objects or bytes);
    -> one bool per proof, each what Proof.verify(circuit, strict=strict) would return -- except that a proof whose
    bytes cannot be parsed is simply False here (on its own it raises): one malformed proof does not keep the others
    from being verified."""
    c = _as_circuit(circuit, wire_counts, ctx)
    n = len(proofs)
    if n == 0:
        return []
    keep = []
    ptrs = (C.c_void_p * n)()
    lens = (C.c_size_t * n)()
    for i, p in enumerate(proofs):
        if isinstance(p, Proof):
            buf, ln = p._buffer()
            ptrs[i] = C.cast(buf, C.c_void_p).value
            keep.append(p)
        else:
            b = bytes(p)
            buf = (C.c_uint8 * max(len(b), 1)).from_buffer_copy(b or b"\0")
            ptrs[i] = C.addressof(buf)
            ln = len(b)
        keep.append(buf)
        lens[i] = ln
    ok = (C.c_int * n)()
    flags = 0 if strict else _lib.RV_VERIFY_REFERENCE_COMPAT
    _lib.check(_lib.lib().rv_verify_batch(c.ctx.handle, c.handle, C.c_size_t(n), ptrs, lens, C.c_uint32(flags), ok))
    return [bool(x) for x in ok]


def prove_batch_device(circuit: "Circuit", wits_gf2, wits_z64=None, seeds=None, ctx: Optional[Context] = None) -> "list[DeviceProof]":
    """rv_prove_batch_device: Proof.new_batch with the proofs left in GPU memory.  -> one DeviceProof (bincode form) per witness,
    all of them views of ONE torch uint8 GPU tensor of batch * stride bytes (stride: the proof length -- 64 + 40 * the circuit's
    record sizes + 2 * 216 * 48 -- rounded up to 256), which every view keeps alive.  Proof b's bytes are those of
    Proof.new_batch(...)[b] for the same witnesses and seeds.  wits_gf2: [B][n] bits; wits_z64: [B][m] words or None; seeds:
    [B][256][16] bytes, None draws them from the OS (the entry point takes no NULL).  Witnesses that are torch GPU tensors
    (`_device_witness`; rows may be strided) are read where they lie (rv_prove_batch_device_wdev)."""
    import os

    import torch

    if not isinstance(circuit, Circuit):
        raise TypeError("prove_batch_device takes a compiled Circuit")
    if ctx is not None and ctx is not circuit.ctx:
        raise ValueError("the circuit was compiled in another context")
    dw = _device_witness(wits_gf2, wits_z64, circuit.ctx, "prove_batch_device", batched=True)
    if dw is None:
        g = np.ascontiguousarray(np.asarray(wits_gf2, dtype=np.uint8))
        if g.ndim != 2:
            raise ValueError("wits_gf2 must be [batch][n_bits]")
        batch = g.shape[0]
    else:
        batch = dw[1]
    if batch == 0:
        return []
    if dw is None:
        z = np.ascontiguousarray(np.asarray(wits_z64 if wits_z64 is not None else np.zeros((batch, 0)), dtype=np.uint64))
        if z.ndim != 2 or z.shape[0] != batch:
            raise ValueError("wits_z64 must be [batch][n_words]")
    if seeds is None:
        seeds = np.frombuffer(os.urandom(batch * TOTAL_REPS * 16), np.uint8)
    s = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint8)).reshape(batch, TOTAL_REPS, 16)
    sz2, sz64 = circuit.record_sizes()
    want = 32 + 4 * 8 + 40 * (sz2 + sz64) + 2 * (TOTAL_REPS - 40) * 48
    stride = (want + 255) & ~255
    out = torch.empty(batch * stride, dtype=torch.uint8, device=f"cuda:{circuit.ctx.device}")
    n = C.c_size_t()
    if dw is not None:
        _lib.check(_lib.lib().rv_prove_batch_device_wdev(circuit.ctx.handle, circuit.handle, C.c_size_t(batch), C.byref(dw[0]), _ptr(s),
                                                         C.c_void_p(out.data_ptr()), C.c_size_t(stride), C.byref(n)))
    else:
        _lib.check(_lib.lib().rv_prove_batch_device(circuit.ctx.handle, circuit.handle, C.c_size_t(batch), _ptr(g), C.c_size_t(g.shape[1]), _ptr(z),
                                                    C.c_size_t(z.shape[1]), _ptr(s), C.c_void_p(out.data_ptr()), C.c_size_t(stride), C.byref(n)))
    if n.value != want:
        raise _lib.ReverieError(7, f"proof length {n.value}, expected {want}")
    proofs = []
    for b in range(batch):  # (views made directly: the call has waited for its stream, a device-wide wait per view is not needed)
        dp = DeviceProof.__new__(DeviceProof)
        dp.lens, dp._comm, dp.ctx = None, None, circuit.ctx
        dp.tensor = out[b * stride:b * stride + want]
        dp._ptr, dp._len = out.data_ptr() + b * stride, want
        proofs.append(dp)
    return proofs


def verify_batch_device(circuit: "Circuit", proofs, strict: bool = True) -> "list[bool]":
    """rv_verify_batch_device: verify_batch on proofs that lie in GPU memory -- DeviceProof objects in bincode form (what
    prove_batch_device returns) or contiguous one-dimensional uint8 GPU tensors on the circuit's device, each starting on a 16-byte
    boundary.  -> one bool per proof, each what verify_batch gives host copies of the same bytes.  A sections-form DeviceProof, a
    CPU tensor or any other object raises TypeError before the library is called (batched sections are not supported)."""
    import sys

    torch = sys.modules.get("torch")
    items = []
    for p in proofs:
        if isinstance(p, DeviceProof):
            if p.lens is not None:
                raise TypeError("verify_batch_device takes bincode-form proofs; a sections-form DeviceProof verifies on its own")
            items.append((p._ptr, p._len, p.ctx.device, p))
        elif torch is not None and isinstance(p, torch.Tensor) and p.device.type == "cuda":
            if p.dtype != torch.uint8 or p.dim() != 1 or not p.is_contiguous():
                raise ValueError(f"verify_batch_device takes contiguous one-dimensional uint8 tensors, got {p.dtype} {tuple(p.shape)}")
            items.append((p.data_ptr(), p.numel(), p.device.index, p))
        else:
            raise TypeError("verify_batch_device takes DeviceProof objects or uint8 torch tensors in GPU memory")
    if not isinstance(circuit, Circuit):
        raise TypeError("verify_batch_device takes a compiled Circuit")
    n = len(items)
    if n == 0:
        return []
    for _, _, dev, _ in items:
        if dev is not None and dev != circuit.ctx.device:
            raise ValueError(f"a proof is on device {dev}, the circuit's context on device {circuit.ctx.device}")
    torch.cuda.synchronize(circuit.ctx.device)  # (the bytes are complete before the library's stream reads them)
    ptrs = (C.c_void_p * n)(*[it[0] for it in items])
    lens = (C.c_size_t * n)(*[it[1] for it in items])
    ok = (C.c_int * n)()
    flags = 0 if strict else _lib.RV_VERIFY_REFERENCE_COMPAT
    _lib.check(_lib.lib().rv_verify_batch_device(circuit.ctx.handle, circuit.handle, C.c_size_t(n), ptrs, lens, C.c_uint32(flags), ok))
    return [bool(x) for x in ok]


# ---- Fiat-Shamir helpers (host) ----
def combine_digests(h) -> bytes:
    h = np.ascontiguousarray(np.asarray(h, dtype=np.uint8)).reshape(TOTAL_REPS, 32)
    out = np.zeros(32, np.uint8)
    _lib.check(_lib.lib().rv_combine_digests(_ptr(h), _ptr(out)))
    return out.tobytes()


def challenge(comm: bytes) -> np.ndarray:
    c = np.frombuffer(bytes(comm), np.uint8).copy()
    out = np.zeros(TOTAL_REPS, np.uint8)
    _lib.check(_lib.lib().rv_challenge(_ptr(c), _ptr(out)))
    return out
