"""rv_compactor_* (wire compaction in windows) -- what holds without a GPU: the seven entry points are declared in the header, exported
by the library and bound in _lib.py, they are pure additions (the ABI version stays 8), rv_compactor_info is mirrored field by field,
and the argument checks answer before any device is touched."""
import ctypes as C
import os
import re

from reverie_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "reverie_amd.h")
NEW = {
    "rv_compactor_begin": "int rv_compactor_begin(rv_ctx *ctx, size_t z64_wires, size_t gf2_wires, rv_compactor **out);",
    "rv_compactor_scan": "int rv_compactor_scan(rv_compactor *c, const rv_op *ops, size_t n_ops, int ops_on_device);",
    "rv_compactor_scan_end": "int rv_compactor_scan_end(rv_compactor *c, int *again, rv_compact_info *info",
    "rv_compactor_feed": "int rv_compactor_feed(rv_compactor *c, const rv_op *ops, size_t n_ops, int ops_on_device, rv_op *d_out);",
    "rv_compactor_rewind": "int rv_compactor_rewind(rv_compactor *c);",
    "rv_compactor_get_info": "int rv_compactor_get_info(const rv_compactor *c, rv_compactor_info *info);",
    "rv_compactor_destroy": "void rv_compactor_destroy(rv_compactor *c);",
}
E_ARG = 9
CTYPES = {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32}


def test_declared_exported_and_bound():
    text = re.sub(r"\s+", " ", open(HEADER).read())
    L = _lib.lib()
    for name, decl in NEW.items():
        assert decl in text, name
        assert name in _lib.SYMBOLS and name in _lib.ARGTYPES, name
        fn = getattr(L, name)
        assert fn.restype is (None if name == "rv_compactor_destroy" else C.c_int) and fn.argtypes == _lib.ARGTYPES[name], name
    assert [len(_lib.ARGTYPES[n]) for n in NEW] == [4, 4, 3, 5, 1, 2, 1]


def test_pure_additions_keep_the_abi_version():
    assert _lib.lib().rv_abi_version() == 8


def test_compactor_info_is_mirrored():
    body = re.search(r"typedef struct rv_compactor_info \{(.*?)\} rv_compactor_info;", open(HEADER).read(), re.S).group(1)
    fields = [(m.group(2), CTYPES[m.group(1)]) for m in re.finditer(r"(uint64_t|uint32_t)\s+(\w+);", body)]
    assert [f[0] for f in fields] == ["total_ops", "state_bytes", "peak_feed_bytes", "scans", "b2a"]
    assert _lib.CompactorInfo._fields_ == fields

    class FromHeader(C.Structure):
        _fields_ = fields

    assert C.sizeof(_lib.CompactorInfo) == C.sizeof(FromHeader) == 32


def test_argument_checks_need_no_device():
    L = _lib.lib()
    out = C.c_void_p()
    assert L.rv_compactor_begin(None, 4, 4, C.byref(out)) == E_ARG and not out.value
    assert L.rv_compactor_begin(C.c_void_p(0x1000), 4, 4, None) == E_ARG  # (the context is not looked at before `out`)
    again, ci, info = C.c_int(7), _lib.CompactInfo(), _lib.CompactorInfo()
    assert L.rv_compactor_scan(None, None, 0, 0) == E_ARG
    assert L.rv_compactor_scan_end(None, C.byref(again), C.byref(ci)) == E_ARG and again.value == 7
    assert L.rv_compactor_feed(None, None, 0, 0, None) == E_ARG
    assert L.rv_compactor_rewind(None) == E_ARG
    assert L.rv_compactor_get_info(None, C.byref(info)) == E_ARG
    L.rv_compactor_destroy(None)
