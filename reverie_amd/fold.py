"""Constants folded in op lists (include/reverie_amd.h: rv_ops_fold / rv_ops_fold_device).

Real statements wire public values into blocks written for secret ones: the IV and the padding block of a SHA-256, the round keys of
a cipher with a public key, a comparison against a public bound.  `fold_ops` rewrites record for record: a gate whose operands are
all known becomes a Const, a Mul with one known operand a MulConst (or a Const 0), an Add or Sub with one known operand an AddConst
or SubConst.  Nothing is dropped, moved or renumbered, and every wire's value stays what it was; `prune_ops` afterwards drops the
Consts nothing reads any more.  The order is fold, then prune, then `compact_wires`.

THE PROOF OF A FOLDED LIST IS THE PROOF OF THAT LIST, not of the original: a folded Mul or B2A no longer contributes to it.  Prover
and verifier both fold, or the folded program is the file that is shipped.

A list that passes through in windows is folded by `DeviceFolder` (rv_folder_*): one forward pass that carries a known
byte and a value per wire index from feed to feed, with the same bytes as `fold_ops` of the whole list for every cutting;
`fold_pieces` wraps a source of pieces, and `fold_windows_host` is the window step's definition on the host."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _lib
from ._window import _DeviceStage, info_dict as _info, input_counts
from .ops import OP_DTYPE, largest_wires, program
from .proof import Context, _device_ops, _is_device_ops, _ptr


def fold_ops(ops, wire_counts: Optional[Tuple[int, int]] = None, ctx: Optional[Context] = None, inplace: bool = False, count_only: bool = False):
    """-> (ops, info): the folded records (as many as went in) and rv_fold_info as a dict.

    Host ops (an OP_DTYPE array or anything `program` takes) go through the forward sweep and need no GPU; wire_counts None means
    `largest_wires(ops)`.  A torch GPU tensor of packed rv_op records (the layouts of `Circuit.from_device_ops`) is folded by kernels
    on the context's GPU: the records come back as a new uint8 tensor [n, 24] on the same device; wire_counts must be given then.
    inplace: the records are written into the argument (an OP_DTYPE array or a GPU tensor), which is returned.  count_only: nothing
    is written -- (None, info).  An op list the compiler would refuse raises the compiler's error."""
    fi = _lib.FoldInfo()
    L = _lib.lib()
    if _is_device_ops(ops):
        if wire_counts is None:
            raise ValueError("fold_ops of a device op list needs wire_counts")
        d_ops, n_ops, ctx = _device_ops(ops, ctx, "fold_ops")
        import torch

        head = (ctx.handle, C.c_void_p(d_ops) if n_ops else None, C.c_size_t(n_ops), C.c_size_t(int(wire_counts[0])), C.c_size_t(int(wire_counts[1])))
        if count_only:
            _lib.check(L.rv_ops_fold_device(*head, None, C.byref(fi)))
            return None, _info(fi)
        out = ops if inplace else torch.empty((n_ops, OP_DTYPE.itemsize), dtype=torch.uint8, device=ops.device)
        _lib.check(L.rv_ops_fold_device(*head, C.c_void_p(d_ops if inplace else out.data_ptr()) if n_ops else None, C.byref(fi)))
        return out, _info(fi)
    if inplace:
        if not (isinstance(ops, np.ndarray) and ops.dtype == OP_DTYPE and ops.flags.c_contiguous and ops.flags.writeable):
            raise ValueError("fold_ops(inplace=True) needs a writable contiguous OP_DTYPE array or a GPU tensor")
    else:
        ops = program(ops) if len(ops) else np.zeros(0, OP_DTYPE)
    if wire_counts is None:
        wire_counts = largest_wires(ops) if len(ops) else (0, 0)
    head = (_ptr(ops), C.c_size_t(len(ops)), C.c_size_t(int(wire_counts[0])), C.c_size_t(int(wire_counts[1])))
    if count_only:
        _lib.check(L.rv_ops_fold(*head, None, C.byref(fi)))
        return None, _info(fi)
    out = ops if inplace else np.empty_like(ops)
    _lib.check(L.rv_ops_fold(*head, _ptr(out), C.byref(fi)))
    return out, _info(fi)


def fold_windows_host(ops, wire_counts: Optional[Tuple[int, int]] = None, cuts=()):
    """-> (ops, info): rv_ops_fold_windows_host -- the forward sweep over the windows [0, cuts[0]), [cuts[0], cuts[1]), ..
    [cuts[-1], len(ops)) with one carried state; no GPU.  Every byte is `fold_ops`'s, whatever the cuts (that is the contract the
    windowed device folder is held to).  cuts: non-decreasing positions, none above len(ops) (ReverieError ARG otherwise)."""
    ops = program(ops) if len(ops) else np.zeros(0, OP_DTYPE)
    if wire_counts is None:
        wire_counts = largest_wires(ops) if len(ops) else (0, 0)
    c = np.ascontiguousarray(np.asarray(list(cuts), dtype=np.int64).reshape(-1))
    if c.size and c.min() < 0:
        raise ValueError("a cut is a position in the list: 0 .. len(ops)")
    c = c.astype(np.uintp)
    fi = _lib.FoldInfo()
    out = np.empty_like(ops)
    _lib.check(_lib.lib().rv_ops_fold_windows_host(_ptr(ops), C.c_size_t(len(ops)), C.c_size_t(int(wire_counts[0])), C.c_size_t(int(wire_counts[1])),
                                                   _ptr(c) if c.size else None, C.c_size_t(c.size), _ptr(out), C.byref(fi)))
    return out, _info(fi)


# ---- the same for a list that passes through in windows (rv_folder_*) ----
KEEP_LOG = 1  # RV_FOLDER_KEEP_LOG


class DeviceFolder(_DeviceStage):
    """rv_folder: `fold_ops` for an op list that arrives in feeds.  feed(ops)... forwards -> the folded records, feed by feed; end()
    -> rv_fold_info; rewind() folds the list again from op 0.  keep_log: every rewritten record is kept in a log on the device, and
    after end() replay(ops, first) turns ANY window of the source into the same window of the folded list, in any order;
    replay_end() closes a round that covered the whole list.  ops: an OP_DTYPE array (uploaded) or a torch GPU tensor of packed
    rv_op records.  wire_counts: (z64, gf2) as stated."""

    _what, _destroy, _info_of = "DeviceFolder", "rv_folder_destroy", (_lib.FolderInfo, "rv_folder_get_info")

    def __init__(self, wire_counts: Tuple[int, int], ctx: Optional[Context] = None, keep_log: bool = False):
        super().__init__(ctx or Context.default())
        _lib.check(_lib.lib().rv_folder_begin(self.ctx.handle, C.c_size_t(int(wire_counts[0])), C.c_size_t(int(wire_counts[1])),
                                              C.c_uint32(KEEP_LOG if keep_log else 0), C.byref(self.handle)))

    def _out(self, n, ops, dev, inplace):
        import torch

        if inplace:
            if not dev:
                raise ValueError("inplace needs a GPU tensor of packed rv_op records")
            return ops
        return torch.empty((n, OP_DTYPE.itemsize), dtype=torch.uint8, device=f"cuda:{self.ctx.device}")

    def feed(self, ops, inplace: bool = False, count_only: bool = False):
        """-> the feed's folded records as a uint8 GPU tensor [n, 24] (inplace: the argument, a GPU tensor, written over; count_only:
        None -- the feed is counted, and logged where the log is kept, and nothing is written)"""
        p, n, dev, _keep = self._ops(ops)
        if count_only:
            _lib.check(_lib.lib().rv_folder_feed(self.handle, p, C.c_size_t(n), C.c_int(dev), None))
            return None
        out = self._out(n, ops, dev, inplace)
        _lib.check(_lib.lib().rv_folder_feed(self.handle, p, C.c_size_t(n), C.c_int(dev), (p if inplace else C.c_void_p(out.data_ptr())) if n else None))
        return out

    def end(self) -> dict:
        """-> rv_fold_info of the pass as a dict (also .info)"""
        fi = _lib.FoldInfo()
        _lib.check(_lib.lib().rv_folder_end(self.handle, C.byref(fi)))
        self.info = _info(fi)
        return self.info

    def rewind(self) -> None:
        _lib.check(_lib.lib().rv_folder_rewind(self.handle))

    def replay(self, ops, first: int, inplace: bool = False):
        """ops: the source's records [first, first + len(ops)) -> the folded list's, as a uint8 GPU tensor [n, 24]"""
        p, n, dev, _keep = self._ops(ops)
        out = self._out(n, ops, dev, inplace)
        _lib.check(_lib.lib().rv_folder_replay(self.handle, p, C.c_size_t(n), C.c_int(dev), C.c_uint64(int(first)),
                                               (p if inplace else C.c_void_p(out.data_ptr())) if n else None))
        return out

    def replay_end(self) -> None:
        _lib.check(_lib.lib().rv_folder_replay_end(self.handle))

    def get_info(self) -> dict:
        """rv_folder_info: total_ops, state_bytes, log_bytes, log_records, peak_feed_bytes, feeds, host_feeds"""
        return super().get_info()


def fold_pieces(pieces, wire_counts: Tuple[int, int], ctx: Optional[Context] = None):
    """-> (pieces2, info) for `pieces` as `stream.prove_streaming_pieces` takes them: a callable that returns a fresh iterator of
    (ops, Input counts).  One counting pass with the log kept runs here.  `pieces2` is such a callable too: every call reads the
    source again and yields (the piece's folded records as a GPU tensor, the source's Input counts -- folding rewrites no Input, so
    they pass through, or are counted where the source gives None); where `pieces` has `.backwards`, `pieces2.backwards()` yields the
    same windows from the last to the first, so the result goes straight into `prune.prune_pieces`.  A pass has to be read to its end
    (it is checked against the folded list then) before the next one begins.  info: rv_fold_info as a dict, with "folder"
    (rv_folder_info) beside it; the folder lives as long as `pieces2` (`pieces2.folder`)."""
    if not callable(pieces):
        raise TypeError("fold_pieces reads the pieces several times: pass a callable that returns a fresh iterator")
    df = DeviceFolder(wire_counts, ctx, keep_log=True)
    try:
        for ops, _ in pieces():
            if ops is not None and len(ops):
                df.feed(ops, count_only=True)
        info = dict(df.end())
    except BaseException:
        df.close()
        raise

    open_round = [False]

    def begin_round():
        if open_round[0]:  # (a pass that was not read to its end: its replays do not count in this one)
            try:
                df.replay_end()
            except _lib.ReverieError:
                pass
        open_round[0] = True

    def end_round():
        open_round[0] = False
        df.replay_end()

    def pieces2():
        begin_round()
        first = 0
        for ops, counts in pieces():
            if ops is None or len(ops) == 0:
                continue
            if counts is None:
                counts = input_counts(ops)
            out = df.replay(ops, first)
            first += len(out)
            yield out, counts
        end_round()

    pieces2.folder = df
    backwards = getattr(pieces, "backwards", None)
    if callable(backwards):
        total = int(info["n_ops"])

        def backwards2():
            begin_round()
            end = total
            for ops, counts in backwards():
                if ops is None or len(ops) == 0:
                    continue
                if counts is None:
                    counts = input_counts(ops)
                n = len(ops) if not _is_device_ops(ops) else len(ops.reshape(-1, OP_DTYPE.itemsize))
                end -= n
                yield df.replay(ops, end), counts
            end_round()

        pieces2.backwards = backwards2
    info["folder"] = df.get_info()
    return pieces2, info
