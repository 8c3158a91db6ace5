"""ctypes binding of libreverie_amd.so (the C-ABI declared in include/reverie_amd.h).

There is NO CPU fallback: if the HIP library is missing, or no gfx950 device is visible,
every compute entry point raises.  (The CPU oracle under oracle/ is test infrastructure
and is never imported from this package.)
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# RV_LIB_PATH: an alternative build of the same library (A/B measurements of kernel variants, tools/)
LIB_PATH = os.environ.get("RV_LIB_PATH") or os.path.join(_HERE, "_build", "libreverie_amd.so")

RV_OK = 0
ERRORS = {
    1: "WITNESS_INVALID", 2: "WITNESS_SHORT", 3: "WIRE_OOB", 4: "PROOF_MALFORMED", 5: "BAD_OP",
    6: "NOMEM", 7: "DEVICE", 8: "UNSUPPORTED", 9: "ARG",
}


class ReverieError(RuntimeError):
    def __init__(self, code: int, detail: str = ""):
        self.code = code
        self.name = ERRORS.get(code, "?")
        super().__init__(f"reverie_amd error {code} ({self.name}){': ' + detail if detail else ''}")


class ShardParts(C.Structure):
    _fields_ = [
        ("gf2_online", C.c_void_p), ("gf2_pre", C.c_void_p), ("z64_online", C.c_void_p), ("z64_pre", C.c_void_p),
        ("gf2_online_len", C.c_size_t), ("gf2_pre_len", C.c_size_t), ("z64_online_len", C.c_size_t),
        ("z64_pre_len", C.c_size_t), ("n_online", C.c_uint32), ("n_pre", C.c_uint32),
    ]


class CircuitInfo(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "n_ops", "gf2_inputs", "gf2_muls", "gf2_asserts", "gf2_linear", "gf2_masks", "z64_inputs", "z64_muls",
        "z64_asserts", "z64_linear", "z64_masks", "b2a", "levels", "device_bytes", "scratch_bytes", "compile_us", "upload_us",
        "gf2_operand_rows", "gf2_rows_written")]


class BristolInfo(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_gates", "n_wires", "n_inputs", "n_outputs", "n_and", "n_xor", "n_inv",
                                          "n_other", "gf2_wires")]


class StreamInfo(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_ops", "chunks", "levels", "gf2_masks", "z64_masks", "gf2_muls", "z64_muls", "wire_store_bytes",
                                          "peak_chunk_bytes", "hash_state_bytes", "proof_bytes")] + [("pass_", C.c_uint32), ("kept_mib", C.c_uint32)]


class EvalStatus(C.Structure):  # rv_eval_status
    _fields_ = [("n_failed", C.c_uint64), ("first_failed_op", C.c_uint64)]


class DevWitness(C.Structure):  # rv_dev_witness: witnesses in the memory of the context's device
    _fields_ = [("gf2", C.c_void_p), ("n_gf2", C.c_size_t), ("stride_gf2", C.c_size_t),
                ("z64", C.c_void_p), ("n_z64", C.c_size_t), ("stride_z64", C.c_size_t)]


class EvalStreamInfo(C.Structure):  # rv_eval_stream_info
    _fields_ = [(n, C.c_uint64) for n in ("n_ops", "chunks", "levels", "wire_store_bytes", "peak_chunk_bytes")]


class CompactInfo(C.Structure):  # rv_compact_info
    _fields_ = [("z64_wires", C.c_uint64), ("gf2_wires", C.c_uint64), ("gf2_pinned", C.c_uint64), ("gf2_zero_wire", C.c_uint32),
                ("z64_zero_wire", C.c_uint32), ("gf2_values", C.c_uint64), ("z64_values", C.c_uint64)]


class CompactorInfo(C.Structure):  # rv_compactor_info
    _fields_ = [("total_ops", C.c_uint64), ("state_bytes", C.c_uint64), ("peak_feed_bytes", C.c_uint64), ("scans", C.c_uint32), ("b2a", C.c_uint32)]


class ProgramInfo(C.Structure):  # rv_program_info
    _fields_ = [(n, C.c_uint64) for n in ("n_ops", "bytes", "z64_wires", "gf2_wires", "n_gf2", "n_z64", "n_b2a", "n_sizehint")]


class ProgramPiece(C.Structure):  # rv_program_piece
    _fields_ = [(n, C.c_uint64) for n in ("first_op", "n_ops", "n_input_gf2", "n_input_z64")]


class BristolPiece(C.Structure):  # rv_bristol_piece
    _fields_ = [(n, C.c_uint64) for n in ("first_op", "n_ops", "n_input_gf2", "first_line", "n_lines")]


class WriterPiece(C.Structure):  # rv_writer_piece
    _fields_ = [(n, C.c_uint64) for n in ("first_op", "n_ops", "file_off", "bytes")]


class LinkBlock(C.Structure):  # rv_link_block
    _fields_ = [("ops", C.c_void_p), ("n_ops", C.c_uint64), ("z64_wires", C.c_uint64), ("gf2_wires", C.c_uint64)]


class LinkDesc(C.Structure):  # rv_link_desc
    _fields_ = [("blocks", C.POINTER(LinkBlock)), ("n_blocks", C.c_uint64), ("block_of", C.c_void_p), ("n_instances", C.c_uint64),
                ("bindings", C.c_void_p), ("n_bindings", C.c_uint64), ("z64_base", C.c_uint64), ("gf2_base", C.c_uint64),
                ("head", C.c_void_p), ("n_head", C.c_uint64), ("tail", C.c_void_p), ("n_tail", C.c_uint64)]


class LinkInfo(C.Structure):  # rv_link_info
    _fields_ = [(n, C.c_uint64) for n in ("n_ops", "n_instances", "n_input_gf2", "n_input_z64", "z64_wires", "gf2_wires")]


class LinkPiece(C.Structure):  # rv_link_piece
    _fields_ = [(n, C.c_uint64) for n in ("first_op", "n_ops", "n_input_gf2", "n_input_z64")]


class PrunerInfo(C.Structure):  # rv_pruner_info
    _fields_ = [(n, C.c_uint64) for n in ("total_ops", "n_kept", "state_bytes", "peak_feed_bytes", "mark_feeds", "host_feeds")]


class PruneInfo(C.Structure):  # rv_prune_info
    _fields_ = [(n, C.c_uint64) for n in ("n_kept", "n_dropped", "dropped_gf2_mul", "dropped_z64_mul", "dropped_b2a", "dropped_gf2_random",
                                          "dropped_z64_random", "dropped_gf2_other", "dropped_z64_other", "unread_gf2_inputs",
                                          "unread_z64_inputs")] + [("device_rounds", C.c_uint32), ("on_device", C.c_uint32)]


class FoldInfo(C.Structure):  # rv_fold_info
    _fields_ = [(n, C.c_uint64) for n in ("n_ops", "n_rewritten", "n_known", "gf2_mul_to_const", "z64_mul_to_const", "gf2_mul_to_linear",
                                          "z64_mul_to_linear", "b2a_to_const", "gf2_other_rewritten", "z64_other_rewritten",
                                          "asserts_known_zero", "asserts_known_nonzero")] + [("device_rounds", C.c_uint32), ("on_device", C.c_uint32)]


class FolderInfo(C.Structure):  # rv_folder_info
    _fields_ = [(n, C.c_uint64) for n in ("total_ops", "state_bytes", "log_bytes", "log_records", "peak_feed_bytes", "feeds", "host_feeds")]


class Z64FRunArgs(C.Structure):  # rv_hook_z64f_run_args
    _fields_ = [("seeds", C.c_void_p), ("omit", C.c_void_p), ("R", C.c_uint32), ("key_path", C.c_uint32), ("first_block", C.c_uint64),
                ("qg0", C.c_uint32), ("qgn", C.c_uint32), ("gates", C.c_void_p), ("n_gates", C.c_size_t), ("levels", C.c_void_p),
                ("n_levels", C.c_size_t), ("runs", C.c_void_p), ("n_runs", C.c_size_t), ("on_words", C.c_uint64), ("pre_words", C.c_uint64),
                ("wit", C.c_void_p), ("n_wit", C.c_size_t), ("sup_in", C.c_void_p), ("sup_corr", C.c_void_p), ("sup_rec", C.c_void_p),
                ("n_in", C.c_size_t), ("n_corr", C.c_size_t), ("n_rec", C.c_size_t), ("sup_r", C.c_uint32), ("reserved", C.c_uint32),
                ("n_ssa", C.c_size_t), ("n_mask_rows", C.c_size_t), ("wmask", C.c_void_p), ("masks", C.c_void_p), ("v", C.c_void_p),
                ("wcorr", C.c_void_p), ("on", C.c_void_p), ("pre", C.c_void_p), ("err", C.c_void_p)]


class Profile(C.Structure):
    _fields_ = [("ms", C.c_double * 8), ("launches", C.c_uint64 * 8), ("calls", C.c_uint64)]


PHASES = ["setup", "masks", "interp", "hash", "join", "open"]


# every symbol include/reverie_amd.h declares (checked by tests/test_abi.py)
SYMBOLS = [
    "rv_strerror", "rv_last_error", "rv_abi_version", "rv_ctx_create", "rv_ctx_destroy", "rv_ctx_sync",
    "rv_circuit_compile", "rv_circuit_compile_ex", "rv_hook_compile_info", "rv_hook_compile_compare", "rv_circuit_destroy", "rv_circuit_get_info", "rv_circuit_early_staging_bytes", "rv_ctx_ops_cache_clear", "rv_prove", "rv_verify", "rv_free",
    "rv_shard_commit", "rv_shard_digests_device", "rv_shard_digests", "rv_shard_open", "rv_shard_destroy",
    "rv_shard_open_device", "rv_combine_digests", "rv_challenge", "rv_assemble_proof", "rv_verify_shard",
    "rv_verify_finish", "rv_hook_prg_blocks", "rv_hook_expand_seed", "rv_hook_sharegen_gf2", "rv_hook_sharegen_z64",
    "rv_hook_blake3", "rv_hook_shard_stream_digests", "rv_ctx_profile", "rv_shard_digests_to_device", "rv_shard_open_size", "rv_shard_open_into", "rv_shard_open_self", "rv_shard_open_gathered",
    "rv_bristol_parse", "rv_circuit_record_sizes", "rv_program_from_bincode", "rv_program_to_bincode", "rv_prove_batch", "rv_prove_device",
    "rv_verify_ex", "rv_verify_shard_ex", "rv_verify_finish_ex", "rv_verify_batch",
    "rv_hook_gf2_reconstruct", "rv_hook_z64_reconstruct", "rv_hook_early_proofs", "rv_hook_open_direct_proofs", "rv_hook_ops_cache_hits", "rv_hook_ops_same", "rv_hook_overlap_commits", "rv_hook_early_plan", "rv_hook_verify_vc_count",
    "rv_stream_begin", "rv_stream_feed", "rv_stream_commit", "rv_stream_finish", "rv_stream_abort", "rv_stream_get_info", "rv_stream_same_cuts",
    "rv_prove_streaming", "rv_prove_ops", "rv_verify_ops", "rv_stream_verify_begin", "rv_stream_verify_finish", "rv_verify_streaming",
    "rv_comm_unique_id", "rv_comm_create", "rv_comm_create_all", "rv_comm_destroy", "rv_prove_sharded", "rv_prove_multi",
    "rv_evaluate", "rv_evaluate_batch", "rv_hook_eval_schedules",
    "rv_eval_stream_begin", "rv_eval_stream_feed", "rv_eval_stream_finish", "rv_eval_stream_get_info", "rv_eval_stream_abort",
    "rv_evaluate_streaming",
    "rv_stream_begin_batch", "rv_stream_commit_batch", "rv_stream_finish_batch", "rv_prove_streaming_batch",
    "rv_stream_verify_begin_batch", "rv_stream_verify_finish_batch", "rv_verify_streaming_batch",
    "rv_verify_shard_groups", "rv_verify_partition", "rv_verify_sharded", "rv_verify_multi", "rv_hook_verify_proof_bytes",
    "rv_circuit_compile_device", "rv_ctx_set_compile_flags", "rv_hook_compile_compare_device", "rv_hook_compile_device_laps",
    "rv_stream_set_compile_flags", "rv_eval_stream_set_compile_flags", "rv_hook_compile_compare_device_chunk", "rv_hook_stream_device_chunks",
    "rv_circuit_compiled_on_device",
    "rv_hook_maskgen",
    "rv_stream_feed_device", "rv_eval_stream_feed_device", "rv_hook_stream_op_traffic", "rv_hook_stream_piece_sums",
    "rv_hook_compile_compare_device_chunk_ex", "rv_hook_compile_device_laps_z64",
    "rv_verify_device", "rv_verify_sections_device", "rv_hook_verify_device_paths", "rv_hook_verify_walk", "rv_hook_verify_schedule",
    "rv_prove_batch_device", "rv_verify_batch_device", "rv_hook_verify_batch_device_paths",
    "rv_prove_wdev", "rv_prove_device_wdev", "rv_prove_batch_wdev", "rv_prove_batch_device_wdev", "rv_evaluate_batch_device",
    "rv_hook_witness_traffic",
    "rv_stream_feed_wdev", "rv_eval_stream_feed_wdev", "rv_stream_finish_device", "rv_stream_finish_batch_device",
    "rv_stream_verify_begin_device", "rv_stream_verify_begin_batch_device",
    "rv_hook_stream_traffic", "rv_hook_stream_verify_device_paths", "rv_hook_stream_wit_sums",
    "rv_hook_extract_bits", "rv_hook_extract_from_bits", "rv_hook_pack_corr_all", "rv_hook_unpack_bits", "rv_hook_extract64", "rv_hook_unpack64",
    "rv_hook_compile_levels", "rv_hook_circuit_levels", "rv_hook_interp_launches",
    "rv_hook_interp64_launches", "rv_hook_z64_fused_grid", "rv_hook_z64_fused_levels", "rv_hook_z64_fused_gates", "rv_hook_z64_fused_run",
    "rv_ops_compact_wires", "rv_ops_compact_wires_device",
    "rv_compactor_begin", "rv_compactor_scan", "rv_compactor_scan_end", "rv_compactor_feed", "rv_compactor_rewind", "rv_compactor_get_info",
    "rv_compactor_destroy",
    "rv_bristol_header", "rv_bristol_parse_device", "rv_hook_bristol_tiles",
    "rv_program_from_bincode_device", "rv_program_to_bincode_device", "rv_hook_bincode_tiles",
    "rv_program_reader_begin", "rv_program_reader_feed", "rv_program_reader_finish", "rv_program_reader_destroy", "rv_hook_program_reader_resume",
    "rv_bristol_header_prefix", "rv_bristol_reader_begin", "rv_bristol_reader_feed", "rv_bristol_reader_header", "rv_bristol_reader_finish",
    "rv_bristol_reader_destroy", "rv_hook_bristol_reader_resume",
    "rv_bristol_write", "rv_bristol_write_device", "rv_hook_bristol_write_tiles",
    "rv_bristol_writer_begin", "rv_bristol_writer_feed", "rv_bristol_writer_finish", "rv_bristol_writer_destroy",
    "rv_program_writer_begin", "rv_program_writer_feed", "rv_program_writer_finish", "rv_program_writer_destroy",
    "rv_witness_parse", "rv_witness_write", "rv_witness_parse_device", "rv_hook_witness_text_tiles", "rv_witness_write_device",
    "rv_witness_reader_begin", "rv_witness_reader_feed", "rv_witness_reader_finish", "rv_witness_reader_destroy",
    "rv_link", "rv_link_plan_create", "rv_link_plan_info", "rv_link_plan_emit", "rv_link_plan_destroy", "rv_hook_link_tiles",
    "rv_ops_prune", "rv_ops_prune_device", "rv_hook_prune_limits", "rv_hook_prune_launches",
    "rv_ops_prune_windows_host", "rv_pruner_begin", "rv_pruner_scan", "rv_pruner_scan_end", "rv_pruner_mark", "rv_pruner_mark_end", "rv_pruner_feed",
    "rv_pruner_rewind", "rv_pruner_get_info", "rv_pruner_destroy",
    "rv_ops_fold", "rv_ops_fold_device", "rv_hook_fold_limits", "rv_hook_fold_launches",
    "rv_ops_fold_windows_host", "rv_folder_begin", "rv_folder_feed", "rv_folder_end", "rv_folder_rewind", "rv_folder_replay", "rv_folder_replay_end",
    "rv_folder_get_info", "rv_folder_destroy",
    "rv_hook_prove_schedule",
    "rv_hook_b3_plan", "rv_hook_b3_chunks", "rv_hook_b3_pair_small", "rv_hook_b3_pair_big_chunks", "rv_hook_b3_tree", "rv_hook_b3_pair_big_tree",
    "rv_hook_b3_incremental", "rv_hook_b3_join",
    "rv_hook_fs_challenge", "rv_hook_open_headers", "rv_hook_open_small", "rv_hook_frame_counts",
    "rv_hook_overlay_rows", "rv_hook_fill_digests", "rv_hook_shard_init", "rv_hook_store_words",
]
_P, _Z = C.c_void_p, C.c_size_t
# argument types of the batched stream entry points (ctypes checks every call against them)
ARGTYPES = {
    "rv_stream_begin_batch": [_P, _Z, _Z, _Z, _P, _Z, C.POINTER(C.c_void_p)],
    "rv_stream_commit_batch": [_P, _P],
    "rv_stream_finish_batch": [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)],
    "rv_prove_streaming_batch": [_P, _P, _Z, _Z, _Z, _Z, _P, _Z, _P, _Z, _P, _Z, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(StreamInfo)],
    "rv_stream_verify_begin_batch": [_P, _Z, _Z, _Z, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), _Z, C.POINTER(C.c_void_p)],
    "rv_stream_verify_finish_batch": [_P, C.c_uint32, C.POINTER(C.c_int)],
    "rv_verify_streaming_batch": [_P, _P, _Z, _Z, _Z, _Z, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_uint32, _Z, C.POINTER(C.c_int),
                                  C.POINTER(StreamInfo)],
    # multi-GPU verification
    "rv_verify_shard_groups": [_P, _P, _P, _Z, _P, C.c_uint32, _P, C.POINTER(C.c_int)],
    "rv_verify_partition": [C.c_int, C.c_int, _P, C.POINTER(C.c_uint32)],
    "rv_verify_sharded": [_P, _P, _P, _Z, C.c_uint32, C.POINTER(C.c_int)],
    "rv_verify_multi": [_P, _P, C.c_int, _P, _Z, C.c_uint32, C.POINTER(C.c_int)],
    "rv_hook_verify_proof_bytes": [],
    # the device compiler
    "rv_circuit_compile_device": [_P, _P, _Z, _Z, _Z, C.c_uint32, C.POINTER(C.c_void_p)],
    "rv_ctx_set_compile_flags": [_P, C.c_uint32],
    "rv_hook_compile_compare_device": [_P, _P, _Z, _Z, _Z, C.c_uint32, C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "rv_hook_compile_device_laps": [C.POINTER(C.c_double)],
    # the device compiler in the streams
    "rv_stream_set_compile_flags": [_P, C.c_uint32],
    "rv_eval_stream_set_compile_flags": [_P, C.c_uint32],
    "rv_hook_compile_compare_device_chunk": [_P, _P, _Z, _Z, _Z, C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "rv_hook_compile_compare_device_chunk_ex": [_P, _P, _Z, _Z, _Z, C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "rv_hook_compile_device_laps_z64": [C.POINTER(C.c_double)],
    "rv_hook_stream_device_chunks": [],
    "rv_circuit_compiled_on_device": [_P, C.POINTER(C.c_int)],
    # streams fed from device memory
    "rv_stream_feed_device": [_P, _P, _Z, _P, _Z, _P, _Z],
    "rv_eval_stream_feed_device": [_P, _P, _Z, _P, _Z, _P, _Z],
    "rv_hook_stream_op_traffic": [C.POINTER(C.c_uint64)],
    "rv_hook_stream_piece_sums": [_P, _P, _Z, C.c_uint64, _Z, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)],
    # verification from device memory
    "rv_verify_device": [_P, _P, _P, _Z, C.c_uint32, C.POINTER(C.c_int)],
    "rv_verify_sections_device": [_P, _P, _P, _P, C.POINTER(C.c_size_t), C.c_uint32, C.POINTER(C.c_int)],
    "rv_hook_verify_device_paths": [C.POINTER(C.c_uint64)],
    "rv_hook_verify_schedule": [C.POINTER(C.c_uint64)],
    "rv_hook_prove_schedule": [C.POINTER(C.c_uint64)],
    "rv_hook_verify_walk": [_P, _Z, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_int)],
    # batches that stay in device memory
    "rv_prove_batch_device": [_P, _P, _Z, _P, _Z, _P, _Z, _P, _P, _Z, C.POINTER(C.c_size_t)],
    "rv_verify_batch_device": [_P, _P, _Z, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_uint32, C.POINTER(C.c_int)],
    "rv_hook_verify_batch_device_paths": [C.POINTER(C.c_uint64)],
    # witnesses taken from device memory, evaluation results left there
    "rv_prove_wdev": [_P, _P, C.POINTER(DevWitness), _P, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)],
    "rv_prove_device_wdev": [_P, _P, C.POINTER(DevWitness), _P, _P, _P, _P, C.POINTER(C.c_size_t)],
    "rv_prove_batch_wdev": [_P, _P, _Z, C.POINTER(DevWitness), _P, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)],
    "rv_prove_batch_device_wdev": [_P, _P, _Z, C.POINTER(DevWitness), _P, _P, _Z, C.POINTER(C.c_size_t)],
    "rv_evaluate_batch_device": [_P, _P, _Z, C.POINTER(DevWitness), _P, _Z, _P, _Z, _P, _P, _P],
    "rv_hook_witness_traffic": [C.POINTER(C.c_uint64)],
    # streams in device memory: witnesses in, proofs out, verification in place
    "rv_stream_feed_wdev": [_P, _P, _Z, C.c_int, C.POINTER(DevWitness)],
    "rv_eval_stream_feed_wdev": [_P, _P, _Z, C.c_int, C.POINTER(DevWitness)],
    "rv_stream_finish_device": [_P, _P, _Z, C.POINTER(C.c_size_t)],
    "rv_stream_finish_batch_device": [_P, _P, _Z, C.POINTER(C.c_size_t)],
    "rv_stream_verify_begin_device": [_P, _Z, _Z, _P, _Z, _Z, C.POINTER(C.c_void_p)],
    "rv_stream_verify_begin_batch_device": [_P, _Z, _Z, _Z, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), _Z, C.POINTER(C.c_void_p)],
    "rv_hook_stream_traffic": [C.POINTER(C.c_uint64)],
    "rv_hook_stream_verify_device_paths": [C.POINTER(C.c_uint64)],
    "rv_hook_stream_wit_sums": [_P, _P, _Z, C.c_uint64, _P, _Z, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)],
    # the mask generators (parity hook)
    "rv_hook_maskgen": [_P, _P, C.c_uint32, _P, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, _P],
    # the opening and unpacking kernels (parity hooks)
    "rv_hook_extract_bits": [_P, _P, C.c_uint64, _P, C.c_uint64, C.c_uint32, C.c_int, _P, _P, _P, C.c_uint64, _P, C.c_uint32, _P, C.POINTER(C.c_uint32)],
    "rv_hook_extract_from_bits": [_P, _P, C.c_uint64, C.c_uint32, _P, _P, C.c_uint32, _P, C.c_uint64, C.POINTER(C.c_uint32)],
    "rv_hook_pack_corr_all": [_P, _P, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, _P],
    "rv_hook_unpack_bits": [_P, _P, C.c_uint64, _P, _P, _P, C.c_uint64, C.c_uint32, C.c_int, C.c_uint32, C.c_uint64, _P],
    "rv_hook_extract64": [_P, _P, C.c_uint64, _P, C.c_uint64, C.c_int, C.c_uint32, _P, _P, C.c_int, C.c_uint32, _P, C.c_uint64],
    "rv_hook_unpack64": [_P, _P, C.c_uint64, _P, _P, _P, C.c_uint64, C.c_uint32, C.c_uint32, _P],
    # which executor runs which level (level table + run plan, launch counters)
    "rv_hook_compile_levels": [_P, _Z, _Z, _Z, C.c_uint32, _P, _Z, C.POINTER(C.c_size_t)],
    "rv_hook_circuit_levels": [_P, _P, _Z, C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "rv_hook_interp_launches": [_P, C.c_int],
    "rv_hook_interp64_launches": [_P, C.c_int],
    "rv_hook_z64_fused_grid": [C.c_uint32] * 6 + [C.POINTER(C.c_uint32)],
    "rv_hook_z64_fused_levels": [_P, _Z, _Z, _Z, C.c_uint32, _P, _Z, C.POINTER(C.c_size_t), C.POINTER(C.c_int)],
    "rv_hook_z64_fused_gates": [_P, _Z, _Z, _Z, C.c_uint32, _P, _Z, C.POINTER(C.c_size_t), _P, _Z, C.POINTER(C.c_size_t), _P, _Z,
                                C.POINTER(C.c_size_t), C.POINTER(C.c_int), _P],
    "rv_hook_z64_fused_run": [_P, C.POINTER(Z64FRunArgs)],
    # wire indices compacted by liveness
    "rv_ops_compact_wires": [_P, _Z, _Z, _Z, _P, C.POINTER(CompactInfo)],
    "rv_ops_compact_wires_device": [_P, _P, _Z, _Z, _Z, _P, C.POINTER(CompactInfo)],
    "rv_compactor_begin": [_P, _Z, _Z, C.POINTER(C.c_void_p)],
    "rv_compactor_scan": [_P, _P, _Z, C.c_int],
    "rv_compactor_scan_end": [_P, C.POINTER(C.c_int), C.POINTER(CompactInfo)],
    "rv_compactor_feed": [_P, _P, _Z, C.c_int, _P],
    "rv_compactor_rewind": [_P],
    "rv_compactor_get_info": [_P, C.POINTER(CompactorInfo)],
    "rv_compactor_destroy": [_P],
    # the Bristol parser on the GPU
    "rv_bristol_header": [_P, _Z, C.c_int, C.POINTER(BristolInfo), C.POINTER(C.c_size_t)],
    "rv_bristol_parse_device": [_P, _P, _Z, C.c_int, C.c_int, _P, _Z, _P, _Z, C.POINTER(C.c_size_t), C.POINTER(BristolInfo)],
    "rv_hook_bristol_tiles": [C.POINTER(C.c_uint32)],
    # program files on the GPU
    "rv_program_from_bincode_device": [_P, _P, _Z, C.c_int, _P, _Z, C.POINTER(C.c_size_t), C.POINTER(ProgramInfo)],
    "rv_program_to_bincode_device": [_P, _P, _Z, _P, _Z, C.POINTER(C.c_size_t)],
    "rv_hook_bincode_tiles": [C.POINTER(C.c_uint32)],
    "rv_program_reader_begin": [_P, C.c_uint64, C.POINTER(_P)],
    "rv_program_reader_feed": [_P, _P, _Z, C.c_int, _P, _Z, C.POINTER(ProgramPiece)],
    "rv_program_reader_finish": [_P, C.POINTER(ProgramInfo)],
    "rv_program_reader_destroy": [_P],
    "rv_hook_program_reader_resume": [_P, C.c_uint64, C.c_uint64],
    # a Bristol text in windows
    "rv_bristol_header_prefix": [_P, _Z, C.c_uint64, C.c_int, C.POINTER(BristolInfo), C.POINTER(C.c_size_t)],
    "rv_bristol_reader_begin": [_P, C.c_uint64, C.c_int, _P, _Z, C.POINTER(_P)],
    "rv_bristol_reader_feed": [_P, _P, _Z, C.c_int, _P, _Z, C.POINTER(BristolPiece)],
    "rv_bristol_reader_header": [_P, C.POINTER(BristolInfo)],
    "rv_bristol_reader_finish": [_P, C.POINTER(BristolInfo)],
    "rv_bristol_reader_destroy": [_P],
    "rv_hook_bristol_reader_resume": [_P, C.c_uint64, C.c_uint64, C.c_uint64],
    # Bristol text and program files written on the GPU, whole and in windows
    "rv_bristol_write": [_P, _Z, C.c_uint64, C.c_uint64, C.POINTER(_P), C.POINTER(C.c_size_t)],
    "rv_bristol_write_device": [_P, _P, _Z, C.c_uint64, C.c_uint64, _P, _Z, C.POINTER(C.c_size_t)],
    "rv_hook_bristol_write_tiles": [C.POINTER(C.c_uint32)],
    "rv_bristol_writer_begin": [_P, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(_P)],
    "rv_bristol_writer_feed": [_P, _P, _Z, C.c_int, _P, _Z, C.POINTER(WriterPiece)],
    "rv_bristol_writer_finish": [_P],
    "rv_bristol_writer_destroy": [_P],
    "rv_program_writer_begin": [_P, C.c_uint64, C.POINTER(_P)],
    "rv_program_writer_feed": [_P, _P, _Z, C.c_int, _P, _Z, C.POINTER(WriterPiece)],
    "rv_program_writer_finish": [_P],
    "rv_program_writer_destroy": [_P],
    # witness text on the host and on the GPU, whole and in windows
    "rv_witness_parse": [_P, _Z, _P, _Z, C.POINTER(C.c_size_t)],
    "rv_witness_write": [_P, _Z, C.c_uint64, _P, _Z, C.POINTER(C.c_size_t)],
    "rv_witness_parse_device": [_P, _P, _Z, C.c_int, _P, _Z, C.POINTER(C.c_size_t), _P, _Z, _P],
    "rv_hook_witness_text_tiles": [C.POINTER(C.c_uint32)],
    "rv_witness_write_device": [_P, _P, _Z, C.c_uint64, _P, _Z, C.POINTER(C.c_size_t)],
    "rv_witness_reader_begin": [_P, C.POINTER(_P)],
    "rv_witness_reader_feed": [_P, _P, _Z, C.c_int, _P, _Z, C.POINTER(C.c_size_t)],
    "rv_witness_reader_finish": [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)],
    "rv_witness_reader_destroy": [_P],
    # programs linked from circuit blocks, on the host and on the GPU
    "rv_link": [C.POINTER(LinkDesc), C.POINTER(_P), C.POINTER(LinkInfo)],
    "rv_link_plan_create": [_P, C.POINTER(LinkDesc), C.c_uint32, C.POINTER(_P)],
    "rv_link_plan_info": [_P, C.POINTER(LinkInfo)],
    "rv_link_plan_emit": [_P, C.c_uint64, C.c_uint64, _P, C.POINTER(LinkPiece)],
    "rv_link_plan_destroy": [_P],
    "rv_hook_link_tiles": [C.POINTER(C.c_uint32)],
    # dead ops dropped, on the host and on the GPU
    "rv_ops_prune": [_P, _Z, _Z, _Z, _P, _Z, _P, _Z, _P, _Z, C.POINTER(C.c_size_t), _P, C.POINTER(PruneInfo)],
    "rv_ops_prune_device": [_P, _P, _Z, _Z, _Z, _P, _Z, _P, _Z, _P, _Z, C.POINTER(C.c_size_t), _P, C.POINTER(PruneInfo)],
    "rv_hook_prune_limits": [C.POINTER(C.c_uint32)],
    "rv_hook_prune_launches": [C.POINTER(C.c_uint64)],
    "rv_ops_fold": [_P, _Z, _Z, _Z, _P, C.POINTER(FoldInfo)],
    "rv_ops_fold_device": [_P, _P, _Z, _Z, _Z, _P, C.POINTER(FoldInfo)],
    "rv_hook_fold_limits": [C.POINTER(C.c_uint32)],
    "rv_hook_fold_launches": [C.POINTER(C.c_uint64)],
    "rv_ops_fold_windows_host": [_P, _Z, _Z, _Z, _P, _Z, _P, C.POINTER(FoldInfo)],
    "rv_folder_begin": [_P, _Z, _Z, C.c_uint32, C.POINTER(C.c_void_p)],
    "rv_folder_feed": [_P, _P, _Z, C.c_int, _P],
    "rv_folder_end": [_P, C.POINTER(FoldInfo)],
    "rv_folder_rewind": [_P],
    "rv_folder_replay": [_P, _P, _Z, C.c_int, C.c_uint64, _P],
    "rv_folder_replay_end": [_P],
    "rv_folder_get_info": [_P, C.POINTER(FolderInfo)],
    "rv_folder_destroy": [_P],
    # the same for a list read in windows
    "rv_ops_prune_windows_host": [_P, _Z, _Z, _Z, _P, _Z, _P, _Z, _P, _Z, _P, _Z, C.POINTER(C.c_size_t), _P, C.POINTER(PruneInfo)],
    "rv_pruner_begin": [_P, _Z, _Z, _P, _Z, _P, _Z, C.POINTER(C.c_void_p)],
    "rv_pruner_scan": [_P, _P, _Z, C.c_int],
    "rv_pruner_scan_end": [_P],
    "rv_pruner_mark": [_P, _P, _Z, C.c_int, C.POINTER(C.c_size_t)],
    "rv_pruner_mark_end": [_P, C.POINTER(PruneInfo)],
    "rv_pruner_feed": [_P, _P, _Z, C.c_int, _P, _Z, C.POINTER(C.c_size_t), _P],
    "rv_pruner_rewind": [_P],
    "rv_pruner_get_info": [_P, C.POINTER(PrunerInfo)],
    "rv_pruner_destroy": [_P],
    # the transcript-hash kernels (parity hooks)
    "rv_hook_b3_plan": [C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)],
    "rv_hook_b3_chunks": [_P, C.c_int, _P, C.c_uint64, C.c_uint32, C.c_uint64, _P, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, _P, C.c_uint64,
                          C.POINTER(C.c_uint32)],
    "rv_hook_b3_pair_small": [_P, _P, C.c_uint64, _P, C.c_uint64, C.c_uint32, _P, C.c_uint32, C.c_uint32, C.c_uint32, _P, C.c_uint64, _P, C.c_uint64, _P, _P,
                              C.c_uint64, C.POINTER(C.c_uint32)],
    "rv_hook_b3_pair_big_chunks": [_P, _P, C.c_uint64, _P, C.c_uint64, _P, C.c_uint32, _P, C.c_uint64, _P, C.c_uint64],
    "rv_hook_b3_tree": [_P, _P, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, _P, C.c_uint64, C.POINTER(C.c_uint32)],
    "rv_hook_b3_pair_big_tree": [_P, _P, C.c_uint64, _P, C.c_uint64, C.c_uint32, _P, _P, C.c_uint64, C.POINTER(C.c_uint32)],
    "rv_hook_b3_incremental": [_P, _P, C.c_uint64, C.c_uint32, C.c_uint32, _P, C.c_uint32, _P, C.c_uint64],
    "rv_hook_b3_join": [_P, _P, C.c_uint32, C.c_uint32, _P, C.c_uint64],
    # the Fiat-Shamir, record-head, framing and set-up kernels (parity hooks)
    "rv_hook_fs_challenge": [_P, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P, _P, _P, _P, _P, _P, _P],
    "rv_hook_open_headers": [_P, C.c_uint32, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_uint64],
    "rv_hook_open_small": [_P, C.c_uint32, _P, _P, _P, _P, _P, _P, _P, _P, C.c_uint64, _P, C.c_uint64, _P, C.c_uint64, _P, C.c_uint64, _P, C.c_uint32, C.c_int,
                           C.c_uint32, _P, C.c_uint64, C.POINTER(C.c_int), _P, C.POINTER(C.c_int)],
    "rv_hook_frame_counts": [_P, _P, C.c_uint64, C.c_uint64, C.c_uint32, _P, C.POINTER(C.c_int)],
    "rv_hook_overlay_rows": [_P, _P, _P, _P, C.c_uint32, C.c_uint32, C.c_int],
    "rv_hook_fill_digests": [_P, _P, C.c_uint64, C.c_uint32, _P],
    "rv_hook_shard_init": [_P, _P, _P, C.c_uint64, C.c_uint32, _P, C.c_uint64, C.c_uint32, _P, C.c_uint64, C.c_uint32, _P, _P],
    "rv_hook_store_words": [_P, _P, C.c_uint32, _P, C.c_uint32, C.c_int, C.c_int, C.POINTER(C.c_int)],
}
RV_LINK_WITNESS = 0xFFFFFFFF  # a binding that leaves the port an Input
RV_LINK_BLOCKS_ON_DEVICE = 1
RV_LINK_TABLES_ON_DEVICE = 2
RV_VERIFY_STRICT = 1
RV_COMPILE_WHOLE_PROVER = 1
RV_COMPILE_KEEP_WIRES = 2  # the circuit keeps every wire's final value form: rv_evaluate can return wire values
RV_COMPILE_DEVICE = 4  # compiled on the GPU (GF(2) programs, plain or -- with WHOLE_PROVER -- lazy sums; anything else by the host compiler): the same circuit
RV_COMPILE_DEVICE_Z64 = 8  # with RV_COMPILE_DEVICE: Z64 ops and SizeHint ops that grow nothing compile on the GPU too (B2A still on the host)
RV_COMPILE_DEVICE_B2A = 32  # with both bits above: B2A ops compile on the GPU too (16 stays an unknown bit)
RV_COMPILE_DEVICE_KEEP_WIRES = 128  # with RV_COMPILE_KEEP_WIRES and RV_COMPILE_DEVICE: KEEP_WIRES programs compile on the GPU too (64 stays an unknown bit)
RV_VERIFY_REFERENCE_COMPAT = 2  # the reference verifier's two unchecked conditions stay unchecked

_lib = None


def _pin_hip_runtime():
    """A process must run ONE HIP runtime.  PyTorch-ROCm ships its own libamdhip64 next to torch/lib, this library
    links the system one; whichever is loaded first wins the SONAME, and if that is the system copy a later
    `import torch` finds no GPU ("No HIP GPUs are available") or corrupts the heap at exit.  So when PyTorch is
    installed its copy is loaded first (without importing torch), and both sides then share it — the arrangement
    bench.py and the multi-GPU path (which import torch first anyway) have always run in."""
    import importlib.util
    import sys

    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ReverieError(7, f"{LIB_PATH} is missing — build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                                  "(make -C reverie_amd/csrc); there is no CPU fallback")
        _pin_hip_runtime()
        L = C.CDLL(LIB_PATH)
        L.rv_strerror.restype = C.c_char_p
        L.rv_last_error.restype = C.c_char_p
        L.rv_abi_version.restype = C.c_uint32
        for name in SYMBOLS:
            fn = getattr(L, name)
            if name in ("rv_ctx_destroy", "rv_circuit_destroy", "rv_shard_destroy", "rv_free", "rv_stream_abort", "rv_comm_destroy",
                        "rv_eval_stream_abort", "rv_program_reader_destroy", "rv_bristol_reader_destroy", "rv_compactor_destroy",
                        "rv_bristol_writer_destroy", "rv_program_writer_destroy", "rv_witness_reader_destroy", "rv_link_plan_destroy",
                        "rv_pruner_destroy", "rv_folder_destroy"):
                fn.restype = None
            elif name in ("rv_hook_early_proofs", "rv_hook_open_direct_proofs", "rv_hook_verify_vc_count", "rv_hook_ops_cache_hits", "rv_hook_overlap_commits",
                          "rv_hook_verify_proof_bytes", "rv_hook_stream_device_chunks"):
                fn.restype = C.c_uint64
            elif name not in ("rv_strerror", "rv_last_error", "rv_abi_version"):
                fn.restype = C.c_int
            if name in ARGTYPES:
                fn.argtypes = ARGTYPES[name]
        _lib = L
    return _lib


def check(rc: int):
    if rc != RV_OK:
        raise ReverieError(rc, lib().rv_last_error().decode() if rc in (6, 7) else "")
