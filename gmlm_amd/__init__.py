"""gmlm_amd — MI355X (gfx950) kernel path behind the GraphTextLM forward/backward of chungimungi/GMLM.

Python host (this package) -> C ABI (include/gmlm_hip.h + gmlm_hip_split.h + gmlm_hip_optim.h, libgmlm_hip.so) -> hand-written HIP kernels.
Importing the package does not need a GPU; calling any operator does, and fails loudly otherwise.
"""
from ._lib import GmlmHipError, LIB_PATH, lib  # noqa: F401
from .dense import mm_bf16x3  # noqa: F401
from .gemma3 import gemma3_encode, gemma3_encode_packed  # noqa: F401
from .gemma2 import gemma2_encode, gemma2_encode_packed  # noqa: F401
from .graph import GraphCache, RelCSR, build_rel_csr  # noqa: F401
from .model import GraphTextLM, TokenizedTexts  # noqa: F401
from .nn import CrossAttention, GraphNorm, MultiScaleFusion, RGCNConv, degree  # noqa: F401
from .optim import FusedAdamW  # noqa: F401
from . import ops as _ops
from .ops import edge_types_from_degree, soft_masking_gnn_input  # noqa: F401

# the public function's earlier spelling, gmlm_amd.ops.mm_bf16x3, for callers written before it moved to dense.py (set here:
# ops imports nothing above it)
_ops.mm_bf16x3 = mm_bf16x3

__all__ = ["GraphTextLM", "TokenizedTexts", "RGCNConv", "GraphNorm", "CrossAttention", "MultiScaleFusion", "degree",
           "soft_masking_gnn_input", "edge_types_from_degree", "mm_bf16x3", "build_rel_csr", "GraphCache", "RelCSR", "lib",
           "GmlmHipError", "LIB_PATH", "FusedAdamW", "gemma3_encode", "gemma3_encode_packed", "gemma2_encode", "gemma2_encode_packed"]
