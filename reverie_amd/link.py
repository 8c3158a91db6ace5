"""Programs linked from circuit blocks (include/reverie_amd.h: rv_link / rv_link_plan_*).

The circuits people have are function blocks -- a SHA-256 compression, an AES-128, a 64-bit adder as Bristol Fashion files -- and a
statement worth proving is many of them wired together.  A `Netlist` is a few `Block`s, a table of instances and, per instance, the
bindings of its input ports: to the witness, or to wires that already exist.  `link_host` gives the linked op list on the host (the
definition; no GPU); a `LinkPlan` writes the same bytes into GPU memory, whole or for any range of ordinals, so that a list that is
too long to exist can still feed `stream.prove_streaming_pieces`, `compact.compact_pieces` and the windowed writers.

A bound port becomes a copy (AddConst 0) of the wire it is bound to: every instance emits exactly its block's records, blocks need
not be in SSA form, and `compact_wires` takes the copies' indices back."""
from __future__ import annotations

import ctypes as C
import sys
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .ops import DOM_Z64, OP_DTYPE, OP_INPUT, largest_wires, program
from .proof import Context, _device_ops, _is_device_ops

WITNESS = _lib.RV_LINK_WITNESS


def _ops(ops) -> np.ndarray:
    return program(ops) if ops is not None and len(ops) else np.zeros(0, OP_DTYPE)


def _info(ci) -> dict:
    d = {n: int(getattr(ci, n)) for n, _ in ci._fields_}
    d["wire_counts"] = (d["z64_wires"], d["gf2_wires"])
    return d


class Block:
    """One function block: an op list with its stated wire counts (z64_wires, gf2_wires) -- the share of the global numbering every
    instance takes.  ops: anything `program` takes, or a torch GPU tensor of packed rv_op records (wire_counts and n_ports must be
    given then: nothing is read back).  Its ports are its Input records in list order, both domains counted together."""

    def __init__(self, ops, wire_counts: Optional[Tuple[int, int]] = None, n_ports: Optional[int] = None, outputs: Optional[Sequence[int]] = None):
        self.on_device = _is_device_ops(ops)
        if self.on_device:
            if wire_counts is None or n_ports is None:
                raise ValueError("a Block of device ops needs wire_counts and n_ports")
            self.ops = ops
            self.n_ports = int(n_ports)
        else:
            self.ops = _ops(ops)
            if wire_counts is None:
                wire_counts = largest_wires(self.ops) if len(self.ops) else (0, 0)
            self.n_ports = int(np.count_nonzero((self.ops["opcode"] == OP_INPUT) & (self.ops["domain"] <= DOM_Z64)))
        self.wire_counts = (int(wire_counts[0]), int(wire_counts[1]))
        self.outputs = [int(w) for w in outputs] if outputs is not None else []

    @classmethod
    def from_bristol(cls, text, format: int = 0, ctx: Optional[Context] = None, device: bool = False) -> "Block":
        """A Bristol Fashion text parsed without expected outputs, on the host or (device=True) with `bristol.parse_device`: the ops
        then stay in GPU memory.  .outputs: the local indices of the last n_outputs wires."""
        from . import bristol

        if device:
            ops, info = bristol.parse_device(text, None, format, device=ctx)
        else:
            ops, info = bristol.parse(text, None, format)
        outs = range(info["n_wires"] - info["n_outputs"], info["n_wires"])
        return cls(ops, info["wire_counts"], n_ports=info["n_inputs"], outputs=outs)

    def __len__(self) -> int:
        return _device_ops(self.ops, None, "Block")[1] if self.on_device else len(self.ops)

    def pruned(self, ctx: Optional[Context] = None) -> "Block":
        """The block without the ops its `.outputs` (GF(2) indices) do not depend on (`prune.prune_ops`: assertions, Inputs and what
        they need stay too): the same ports, wire counts and outputs, so it takes the original's place in a `Netlist`.  A device block
        is pruned where it lies.  .prune_info: rv_prune_info as a dict.  The linked program is another program: its proof is not the
        proof of the one linked from the unpruned block."""
        from .prune import prune_ops

        ops, info, _ = prune_ops(self.ops, self.wire_counts, outputs_gf2=self.outputs, ctx=ctx)
        b = Block(ops, self.wire_counts, n_ports=self.n_ports, outputs=self.outputs)
        b.prune_info = info
        return b

    def folded(self, ctx: Optional[Context] = None) -> "Block":
        """The block with the constants of its own records folded (`fold.fold_ops`: a Mul by a Const becomes a MulConst, a gate of
        known operands a Const; a value bound through a port or put on a wire by a netlist's `head` is not known here): the same
        ports, wire counts and outputs, record for record, so it takes the original's place in a `Netlist`.  A device block is folded
        where it lies, into a new tensor.  .fold_info: rv_fold_info as a dict.  `.folded().pruned()` then drops the Consts nothing
        reads any more.  The linked program is another program: its proof is not the proof of the one linked from the unfolded block."""
        from .fold import fold_ops

        ops, info = fold_ops(self.ops, self.wire_counts, ctx=ctx)
        b = Block(ops, self.wire_counts, n_ports=self.n_ports, outputs=self.outputs)
        b.fold_info = info
        return b


class Instance:
    """What `Netlist.add` returns: where instance `index` lies in the global numbering."""

    def __init__(self, index: int, block: Block, z64_base: int, gf2_base: int):
        self.index, self.block, self.z64_base, self.gf2_base = index, block, z64_base, gf2_base

    def wire(self, local: int, domain: str = "gf2") -> int:
        """the global index of the block's wire `local`"""
        return int(local) + (self.gf2_base if domain == "gf2" else self.z64_base)

    @property
    def outputs(self):
        return [self.gf2_base + w for w in self.block.outputs]


class Netlist:
    """blocks, instances and bindings (rv_link_desc).  head / tail: op lists in global numbering, copied as they are (constants and
    global inputs; the assertions on outputs).  The bases -- the first wire index of instance 0 per domain -- default to the head's
    wire counts."""

    def __init__(self, blocks: Sequence[Block], head=None, z64_base: Optional[int] = None, gf2_base: Optional[int] = None):
        self.blocks = [b if isinstance(b, Block) else Block(b) for b in blocks]
        self.head, self.tail = _ops(head), _ops(None)
        hz, hg = largest_wires(self.head) if len(self.head) else (0, 0)
        self.z64_base = int(hz if z64_base is None else z64_base)
        self.gf2_base = int(hg if gf2_base is None else gf2_base)
        self._block_of, self._bindings = [], []
        self._z, self._g = self.z64_base, self.gf2_base
        self.block_of = self.bindings = None  # the tables, once they are arrays (from_arrays, or the lists frozen by _tables)

    def add(self, block_index: int, bindings: Sequence[int]) -> Instance:
        """one more instance of blocks[block_index]; bindings: one entry per port, WITNESS or a global wire index of the port's domain"""
        if self.block_of is not None:
            raise ValueError("the tables of this Netlist are arrays: add() builds lists")
        b = self.blocks[block_index]
        if len(bindings) != b.n_ports:
            raise ValueError(f"block {block_index} has {b.n_ports} ports, got {len(bindings)} bindings")
        inst = Instance(len(self._block_of), b, self._z, self._g)
        self._block_of.append(int(block_index))
        self._bindings.extend(int(v) for v in bindings)
        self._z, self._g = self._z + b.wire_counts[0], self._g + b.wire_counts[1]
        return inst

    def set_tail(self, ops) -> None:
        self.tail = _ops(ops)

    @classmethod
    def from_arrays(cls, blocks, block_of, bindings, head=None, tail=None, z64_base: Optional[int] = None, gf2_base: Optional[int] = None) -> "Netlist":
        """The tables as arrays: uint32 numpy arrays, or contiguous torch GPU tensors of 4-byte integers (int32 or uint32 holding the
        uint32 values; both tables on the same side).  A Python loop over 10^6 instances is not the interface."""
        nl = cls(blocks, head, z64_base, gf2_base)
        nl.set_tail(tail)
        dev = _is_device_ops(block_of), _is_device_ops(bindings)
        if dev[0] != dev[1]:
            raise ValueError("block_of and bindings must both be host arrays or both GPU tensors")
        if dev[0]:
            for t in (block_of, bindings):
                if t.device.type != "cuda" or t.element_size() != 4 or t.is_floating_point() or not t.is_contiguous() or t.dim() != 1:
                    raise ValueError("a table tensor must be a contiguous 1-D GPU tensor of 4-byte integers")
            nl.block_of, nl.bindings = block_of, bindings
        else:
            nl.block_of = np.ascontiguousarray(np.asarray(block_of, dtype=np.uint32).reshape(-1))
            nl.bindings = np.ascontiguousarray(np.asarray(bindings, dtype=np.uint32).reshape(-1))
        return nl

    # ---- the descriptor ----
    def _tables(self):
        if self.block_of is not None:
            return self.block_of, self.bindings
        return np.asarray(self._block_of, dtype=np.uint32), np.asarray(self._bindings, dtype=np.uint32)

    def _desc(self, ctx: Optional[Context], host_only: bool):
        """-> (rv_link_desc, flags, context or None, what keeps the memory alive)"""
        keep = []
        flags = 0
        blocks_dev = [b.on_device for b in self.blocks]
        if any(blocks_dev):
            if host_only:
                raise ValueError("link_host needs host blocks")
            if not all(blocks_dev):
                raise ValueError("the blocks must all be host arrays or all GPU tensors")
            flags |= _lib.RV_LINK_BLOCKS_ON_DEVICE
        arr = (_lib.LinkBlock * max(len(self.blocks), 1))()
        for k, b in enumerate(self.blocks):
            if b.on_device:
                p, n, ctx = _device_ops(b.ops, ctx, "Netlist")
            else:
                p, n = (b.ops.ctypes.data if len(b.ops) else None), len(b.ops)
            arr[k] = _lib.LinkBlock(p, n, b.wire_counts[0], b.wire_counts[1])
            keep.append(b.ops)
        block_of, bindings = self._tables()
        if _is_device_ops(block_of):
            if host_only:
                raise ValueError("link_host needs host tables")
            import torch

            flags |= _lib.RV_LINK_TABLES_ON_DEVICE
            ctx = ctx or Context.default()
            for t in (block_of, bindings):
                if t.device.index is not None and t.device.index != ctx.device:
                    raise ValueError(f"a table is on {t.device}, the context on device {ctx.device}")
            torch.cuda.synchronize(block_of.device)
            p_of, p_bind = block_of.data_ptr() if block_of.numel() else None, bindings.data_ptr() if bindings.numel() else None
            n_of, n_bind = block_of.numel(), bindings.numel()
        else:
            p_of, p_bind = (block_of.ctypes.data if block_of.size else None), (bindings.ctypes.data if bindings.size else None)
            n_of, n_bind = block_of.size, bindings.size
        keep += [arr, block_of, bindings, self.head, self.tail]
        d = _lib.LinkDesc(C.cast(arr, C.POINTER(_lib.LinkBlock)), len(self.blocks), p_of, n_of, p_bind, n_bind, self.z64_base, self.gf2_base,
                          self.head.ctypes.data if len(self.head) else None, len(self.head), self.tail.ctypes.data if len(self.tail) else None,
                          len(self.tail))
        return d, flags, ctx, keep

    def link_host(self, info_only: bool = False):
        """rv_link -> (the linked list as an OP_DTYPE array, info); info: rv_link_info as a dict, with "wire_counts" beside it.
        info_only: (None, info) -- nothing is written."""
        d, _, _, _keep = self._desc(None, True)
        ops, li = C.c_void_p(), _lib.LinkInfo()
        _lib.check(_lib.lib().rv_link(C.byref(d), None if info_only else C.byref(ops), C.byref(li)))
        info = _info(li)
        if info_only:
            return None, info
        out = np.frombuffer(C.string_at(ops, info["n_ops"] * OP_DTYPE.itemsize), dtype=OP_DTYPE).copy()
        _lib.lib().rv_free(ops)
        return out, info

    def plan(self, ctx: Optional[Context] = None) -> "LinkPlan":
        return LinkPlan(self, ctx)


class LinkPlan:
    """rv_link_plan: the linked list of a `Netlist` from kernels, whole or for any range of ordinals, any number of times.  The plan
    holds its own device copy of the netlist; errors are `link_host`'s."""

    def __init__(self, netlist: Netlist, ctx: Optional[Context] = None):
        d, flags, ctx2, _keep = netlist._desc(ctx, False)
        self.ctx = ctx2 or ctx or Context.default()
        self.handle = C.c_void_p()
        _lib.check(_lib.lib().rv_link_plan_create(self.ctx.handle, C.byref(d), C.c_uint32(flags), C.byref(self.handle)))
        li = _lib.LinkInfo()
        _lib.check(_lib.lib().rv_link_plan_info(self.handle, C.byref(li)))
        self.info = _info(li)
        self.last_piece = None

    def emit(self, first: int, n: int, out=None):
        """records first .. first + n - 1 as a uint8 GPU tensor [n, 24] (or into `out`, a GPU tensor of at least n records);
        .last_piece: the range's (n_input_gf2, n_input_z64)"""
        import torch

        if out is None:
            out = torch.empty((int(n), OP_DTYPE.itemsize), dtype=torch.uint8, device=f"cuda:{self.ctx.device}")
        else:
            _, cap, _ = _device_ops(out, self.ctx, "LinkPlan.emit")
            if cap < n:
                raise ValueError(f"out holds {cap} records, the range {n}")
        piece = _lib.LinkPiece()
        _lib.check(_lib.lib().rv_link_plan_emit(self.handle, C.c_uint64(int(first)), C.c_uint64(int(n)), C.c_void_p(out.data_ptr()) if n else None,
                                                C.byref(piece)))
        self.last_piece = (int(piece.n_input_gf2), int(piece.n_input_z64))
        return out

    def link_device(self):
        """the whole list (in calls of less than 2^28 records)"""
        import torch

        n = self.info["n_ops"]
        out = torch.empty((n, OP_DTYPE.itemsize), dtype=torch.uint8, device=f"cuda:{self.ctx.device}")
        step = (1 << 28) - 256
        for first in range(0, n, step):
            self.emit(first, min(step, n - first), out[first:first + min(step, n - first)])
        return out

    def pieces(self, window_ops: int):
        """-> a callable that returns a fresh iterator of (tensor, (n_input_gf2, n_input_z64)) over the list in windows of window_ops
        records: the shape `stream.prove_streaming_pieces`, `verify_streaming_pieces`, `evaluate_streaming_pieces`,
        `compact.compact_pieces`, `bristol.write_device` and `program_file.write_device` take.  The callable's `.backwards` is such
        a callable over the same windows from the last to the first (`prune.prune_pieces` marks from it)"""
        if window_ops <= 0 or window_ops >= 1 << 28:
            raise ValueError("window_ops must lie in [1, 2^28)")

        def windows(firsts):
            n = self.info["n_ops"]
            for first in firsts:
                t = self.emit(first, min(window_ops, n - first))
                yield t, self.last_piece

        def it():
            return windows(range(0, self.info["n_ops"], window_ops))

        def backwards():
            return windows(reversed(range(0, self.info["n_ops"], window_ops)))

        it.backwards = backwards
        return it

    def close(self) -> None:
        """gives the plan's device memory back to its context (a context that was closed first took its memory with it)"""
        if self.handle:
            if self.ctx.handle:
                _lib.lib().rv_link_plan_destroy(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        if sys.is_finalizing():  # (finalisers run in no order then: the context and the runtime may be gone)
            return
        try:
            self.close()
        except Exception:
            pass
