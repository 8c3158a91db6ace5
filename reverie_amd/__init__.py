"""reverie_amd — MI355X-native KKW (MPC-in-the-head) prover/verifier hot path.

Public surface mirrors the reference's `Proof` API (see proof.py) over the C-ABI in
include/reverie_amd.h; `ops` builds gate streams.
"""
from .ops import B2A, GF2, Z64, SizeHint, largest_wires, program  # noqa: F401
from .proof import Circuit, Context, DeviceEvaluation, DeviceProof, Evaluation, Proof, challenge, combine_digests, evaluate_composite_program, prove_batch_device, verify_batch, verify_batch_device  # noqa: F401
from .stream import (StreamingBatchProver, StreamingBatchVerifier, StreamingEvaluator, StreamingProver, StreamingVerifier,  # noqa: F401
                     evaluate_streaming, prove_streaming, prove_streaming_batch, verify_streaming, verify_streaming_batch)
from .compact import compact_wires  # noqa: F401
from .prune import prune_ops  # noqa: F401
from .fold import fold_ops  # noqa: F401
from .link import Block, LinkPlan, Netlist  # noqa: F401
from ._lib import ReverieError  # noqa: F401
