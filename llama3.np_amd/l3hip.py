"""ctypes binding to libllama3hip.so (C ABI: include/llama3hip.h).

This is the only module that touches the native library.  It has no CPU
fallback: if the shared library is missing, ``lib()`` raises, and every device
entry point raises ``RuntimeError(l3_last_error())`` on a non-zero return.
Loading the library needs no GPU (it only resolves symbols); calling a compute
entry point without a HIP device fails loudly.
"""

import ctypes
import os
import re
from typing import List, Optional

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# L3_LIB_PATH: another build of the same library (kernel A/B runs in one box call, tools/ab_lib.sh);
# the product always loads the in-tree build
LIB_PATH = os.environ.get("L3_LIB_PATH") or os.path.join(HERE, "csrc", "libllama3hip.so")
HEADER = os.path.join(os.path.dirname(HERE), "include", "llama3hip.h")

# weight kinds / kernel ids (mirror the enums in include/llama3hip.h)
W_EMBED, W_Q, W_K, W_V, W_O, W_GATE, W_UP, W_DOWN = range(8)
W_ATTN_NORM, W_FFN_NORM, W_FINAL_NORM, W_LM_HEAD = 8, 9, 10, 11
KERNELS = ["embed", "qkv", "attn", "oproj", "gateup", "down", "lmhead", "argmax", "gather", "embed_qkv", "ffn"]


class Dims(ctypes.Structure):
    _fields_ = [
        ("dim", ctypes.c_int32),
        ("n_layers", ctypes.c_int32),
        ("n_heads", ctypes.c_int32),
        ("n_kv_heads", ctypes.c_int32),
        ("vocab_size", ctypes.c_int32),
        ("hidden_dim", ctypes.c_int32),
        ("max_seq_len", ctypes.c_int32),
        ("max_batch_size", ctypes.c_int32),
        ("norm_eps", ctypes.c_float),
    ]


_P = ctypes.c_void_p
_I32 = ctypes.c_int32
_I64 = ctypes.c_int64
_SZ = ctypes.c_size_t
_F = ctypes.c_float

_SIGNATURES = {
    "l3_last_error": (ctypes.c_char_p, []),
    "l3_device_count": (ctypes.c_int, [_P]),
    "l3_version": (ctypes.c_int, [_P, _P]),
    "l3_source_hash": (ctypes.c_char_p, []),
    "l3_host_alloc": (ctypes.c_int, [_SZ, _P]),
    "l3_host_free": (ctypes.c_int, [_P]),
    "l3_create": (ctypes.c_int, [_I32, _P, _P]),
    "l3_create_kv": (ctypes.c_int, [_I32, _P, _I32, _P]),
    "l3_kv_info": (ctypes.c_int, [_P, _P, _P]),
    "l3_cache_read_host": (ctypes.c_int, [_P, _I32, _I32, _I32, _I32, _P, _P]),
    "l3_op_attn_decode_ragged_kv_host": (ctypes.c_int, [_P, _P, _P, _P, _I32, _P, _P, _P, _P, _I32, _I32, _I32, _I32,
                                                        _I32, _I32, _I32, _P]),
    "l3_op_attn_extend_ragged_kv_host": (ctypes.c_int, [_P, _P, _P, _P, _I32, _P, _P, _P, _P, _I32, _I32, _I32, _I32,
                                                        _I32, _I32, _P]),
    "l3_destroy": (ctypes.c_int, [_P]),
    "l3_upload_weight": (ctypes.c_int, [_P, _I32, _I32, _P, _I64, _I64]),
    "l3_finalize": (ctypes.c_int, [_P]),
    "l3_reset_cache": (ctypes.c_int, [_P]),
    "l3_forward_host": (ctypes.c_int, [_P, _P, _I32, _I32, _I32, _P]),
    "l3_forward_dev": (ctypes.c_int, [_P, _P, _I32, _I32, _I32, _P]),
    "l3_score_host": (ctypes.c_int, [_P, _P, _P, _I32, _I32, _I32, _P, _P]),
    "l3_set_score_workspace": (ctypes.c_int, [_P, _I64]),
    "l3_greedy_step_host": (ctypes.c_int, [_P, _P, _I32, _I32, _I32, _P, _P]),
    "l3_layer_forward_host": (ctypes.c_int, [_P, _I32, _P, _I32, _I32, _I32, _P]),
    "l3_greedy_generate_host": (ctypes.c_int, [_P, _P, _I32, _I32, _I32, _P]),
    "l3_greedy_generate_values_host": (ctypes.c_int, [_P, _P, _I32, _I32, _I32, _P, _P]),
    "l3_ragged_forward_host": (ctypes.c_int, [_P, _P, _P, _I32, _I32, _P]),
    "l3_ragged_generate_host": (ctypes.c_int, [_P, _P, _P, _I32, _I32, _I32, _P, _I32, _P, _P]),
    "l3_set_ragged_attn_split": (ctypes.c_int, [_P, _I32, _I32]),
    "l3_ragged_attn_info": (ctypes.c_int, [_P, _P, _P, _P, _P]),
    "l3_op_attn_decode_ragged_host": (ctypes.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32,
                                                     _I32, _I32, _P]),
    "l3_ragged_extend_host": (ctypes.c_int, [_P, _P, _P, _P, _I32, _I32, _P]),
    "l3_ragged_generate_from_host": (ctypes.c_int, [_P, _P, _P, _P, _I32, _I32, _I32, _P, _I32, _P, _P]),
    "l3_cache_copy_rows": (ctypes.c_int, [_P, _I32, _P, _I32, _I32]),
    "l3_op_attn_extend_ragged_host": (ctypes.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32,
                                                     _I32, _P]),
    "l3_ragged_generate_spec_host": (ctypes.c_int, [_P, _P, _P, _P, _I32, _I32, _I32, _P, _I32, _P, _P, _I32, _I32,
                                                    _I32, _I32, _P, _P, _P, _P, _P]),
    "l3_ragged_verify_host": (ctypes.c_int, [_P, _P, _P, _P, _I32, _I32, _P, _P]),
    "l3_op_spec_draft_host": (ctypes.c_int, [_P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _P, _P]),
    "l3_attention_forward_host": (ctypes.c_int, [_P, _I32, _P, _I32, _I32, _I32, _P]),
    "l3_op_softmax_host": (ctypes.c_int, [_P, _P, _I64, _I64, _P]),
    "l3_op_argmax_host": (ctypes.c_int, [_P, _P, _I64, _I64, _P]),
    "l3_op_sample_host": (ctypes.c_int, [_P, _P, _I64, _I64, _F, _I32, _F, _P, ctypes.c_uint64, _I32, _I32, _P]),
    "l3_set_sampling": (ctypes.c_int, [_P, _F, _I32, _F, ctypes.c_uint64]),
    "l3_get_sampling": (ctypes.c_int, [_P, _P, _P, _P, _P]),
    "l3_sample_uniform": (ctypes.c_int, [ctypes.c_uint64, _I32, _I32, _P]),
    "l3_op_silu_host": (ctypes.c_int, [_P, _P, _I64, _P]),
    "l3_op_rmsnorm_host": (ctypes.c_int, [_P, _P, _P, _I64, _I64, _F, _P]),
    "l3_op_rope_host": (ctypes.c_int, [_P, _P, _I32, _I32, _I32, _I32, _P, _P, _P]),
    "l3_op_ffn_host": (ctypes.c_int, [_P, _P, _I64, _I32, _I32, _P, _P, _P, _P]),
    "l3_op_linear_host": (ctypes.c_int, [_P, _P, _I64, _I32, _I32, _P, _P]),
    "l3_op_linear_logprob_host": (ctypes.c_int, [_P, _P, _I64, _I32, _I32, _P, _P, _P, _P, _P]),
    "l3_dev_alloc": (ctypes.c_int, [_P, _SZ, _P]),
    "l3_dev_free": (ctypes.c_int, [_P, _P]),
    "l3_h2d": (ctypes.c_int, [_P, _P, _P, _SZ]),
    "l3_d2h": (ctypes.c_int, [_P, _P, _P, _SZ]),
    "l3_synchronize": (ctypes.c_int, [_P]),
    "l3_set_batch_split": (ctypes.c_int, [_P, _I32, _I64]),
    "l3_set_gemm_x6": (ctypes.c_int, [_P, _I32]),
    "l3_set_embed_qkv": (ctypes.c_int, [_P, _I32, _I64]),
    "l3_set_ffn_fused": (ctypes.c_int, [_P, _I32]),
    "l3_op_ffn_block_host": (ctypes.c_int, [_P, _P, _I64, _I32, _I32, _P, _P, _P, _I32, _I32, _P]),
    "l3_set_weight_bf16": (ctypes.c_int, [_P, _I32]),
    "l3_weight_bf16_info": (ctypes.c_int, [_P, _P, _P, _P]),
    "l3_set_weight_bf16_rows": (ctypes.c_int, [_P, _I32, _I64]),
    "l3_weight_bf16_rows_info": (ctypes.c_int, [_P, _P, _P, _P]),
    "l3_op_linear_bf16_rows_host": (ctypes.c_int, [_P, _P, _I64, _I32, _I32, _P, _P, _F, _P]),
    "l3_op_to_bf16_host": (ctypes.c_int, [_P, _P, _I64, _P, _P]),
    "l3_set_weight_fp8": (ctypes.c_int, [_P, _I32]),
    "l3_weight_fp8_info": (ctypes.c_int, [_P, _P, _P, _P, _P]),
    "l3_op_to_fp8_rows_host": (ctypes.c_int, [_P, _P, _I64, _I32, _P, _P, _P]),
    "l3_op_linear_fp8_host": (ctypes.c_int, [_P, _P, _I64, _I32, _I32, _P, _P, _P, _F, _P, _P]),
    "l3_op_linear_fp8_rows_host": (ctypes.c_int, [_P, _P, _I64, _I32, _I32, _P, _P, _P, _F, _P, _P]),
    "l3_op_linear_bf16_host": (ctypes.c_int, [_P, _P, _I64, _I32, _I32, _P, _P, _F, _P]),
    "l3_op_gemm_host": (ctypes.c_int, [_P, _P]),
    "l3_op_decode_gemm_host": (ctypes.c_int, [_P, _P]),
    "l3_op_decode_persist_host": (ctypes.c_int, [_P, _P]),
    "l3_op_argmax_parts_host": (ctypes.c_int, [_P, _P, _I32, _I32, _I32, _P, _P]),
    "l3_op_kv_restore_host": (ctypes.c_int, [_P, _P, _I64, _P, _I32, _I32, _I32, _I32, _I32]),
    "l3_op_attention_host": (ctypes.c_int, [_P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _P, _I32,
                                            _P, _I64, _P]),
    "l3_set_last_layer_rows": (ctypes.c_int, [_P, _I32]),
    "l3_kernel_timing": (ctypes.c_int, [_P, _I32]),
    "l3_kernel_stats": (ctypes.c_int, [_P, _P, _P]),
    "l3_decode_stats": (ctypes.c_int, [_P, _P, _P]),
    "l3_decode_persistent": (ctypes.c_int, [_P, _P]),
    "l3_decode_recoveries": (ctypes.c_int, [_P, _P]),
    "l3_set_decode_horizon": (ctypes.c_int, [_P, _I32]),
    "l3_comm_unique_id": (ctypes.c_int, [_P]),
    "l3_comm_init": (ctypes.c_int, [_P, _I32, _I32, _P]),
    "l3_comm_gather_logits": (ctypes.c_int, [_P, _P, _P, _P, _I32]),
    "l3_comm_gather_argmax": (ctypes.c_int, [_P, _P, _P, _P, _I32]),
    "l3_comm_barrier": (ctypes.c_int, [_P]),
    "l3_comm_allreduce_max": (ctypes.c_int, [_P, _P]),
    "l3_comm_info": (ctypes.c_int, [_P, _P, _P, _P, _P, _I64]),
    "l3_comm_set_overlap": (ctypes.c_int, [_P, _I32]),
    "l3_group_create": (ctypes.c_int, [_I32, _P, _P, _P]),
    "l3_group_destroy": (ctypes.c_int, [_P]),
    "l3_group_context": (ctypes.c_int, [_P, _I32, _P]),
    "l3_group_upload_weight": (ctypes.c_int, [_P, _I32, _I32, _P, _I64, _I64]),
    "l3_group_finalize": (ctypes.c_int, [_P]),
    "l3_group_forward_host": (ctypes.c_int, [_P, _P, _I32, _I32, _I32, _P]),
    "l3_group_forward_dev": (ctypes.c_int, [_P, _P, _I32, _I32, _I32, _P]),
    "l3_group_greedy_step_host": (ctypes.c_int, [_P, _P, _I32, _I32, _I32, _P]),
    "l3_group_synchronize": (ctypes.c_int, [_P]),
    "l3_device_check_counts": (ctypes.c_int, [_P, _P, _P]),
    "l3_device_check_selftest": (ctypes.c_int, [_P]),
}

BUSID_LEN = 16  # L3_BUSID_LEN


class GemmOp(ctypes.Structure):
    """l3_gemm_op (include/llama3hip.h)."""
    _fields_ = [
        ("struct_size", _I32), ("epi", _I32), ("M", _I32), ("N", _I32), ("K", _I32), ("norm", _I32),
        ("eps", _F), ("q_scale", _F),
        ("x", _P), ("w", _P), ("norm_w", _P), ("a_rows", _P), ("x_rows", _I64),
        ("c", _P), ("c_rows", _I64), ("res_src", _P), ("res_rows", _P), ("res_src_rows", _I64),
        ("L", _I32), ("start_pos", _I32), ("H", _I32), ("KVH", _I32), ("HD", _I32), ("Smax", _I32),
        ("col_base", _I32), ("cache_B", _I32),
        ("rope_cos", _P), ("rope_sin", _P), ("q_out", _P), ("q_rows", _I64), ("cache_k", _P), ("cache_v", _P),
        ("ws_floats", _I64), ("wb_min_bytes", _I64),
        ("force_skinny", _I32), ("force_tiled", _I32), ("x6", _I32), ("bf16", _I32), ("wb_rows", _I32),
        ("route", _I32 * 8),
    ]


class DecStateIO(ctypes.Structure):
    """l3_dec_state_io (include/llama3hip.h)."""
    _fields_ = [
        ("struct_size", _I32), ("pos", _I32), ("hist_base", _I32), ("hist_cap", _I32), ("arrive", ctypes.c_uint32),
        ("pad", _I32), ("hist", _P), ("hist_val", _P), ("hist_len", _I64),
    ]


class DecodeGemmOp(ctypes.Structure):
    """l3_decode_gemm_op (include/llama3hip.h)."""
    _fields_ = [
        ("struct_size", _I32), ("storage", _I32), ("g", GemmOp),
        ("wq_codes", _P), ("wq_scale", _P), ("parts", _P), ("parts_rows", _I64), ("x_out", _P), ("x_out_rows", _I64),
        ("amax_part", _P), ("amax_rows", _P), ("amax_rows_rows", _I64), ("amax_in", _P), ("amax_ids", _P),
        ("state", ctypes.POINTER(DecStateIO)), ("kv_bak", _P),
        ("nparts", _I32), ("amax_part_n", _I32), ("amax_blocks", _I32), ("amax_nct", _I32), ("amax_in_n", _I32),
        ("pos_adv", _I32), ("pos_dev", _I32), ("pad", _I32),
    ]


class DecodePersistOp(ctypes.Structure):
    """l3_decode_persist_op (include/llama3hip.h)."""
    _fields_ = [
        ("struct_size", _I32), ("token", _I32), ("steps", _I32), ("use_kv_bak", _I32),
        ("state", ctypes.POINTER(DecStateIO)), ("gran", _P), ("gran_n", _I64), ("lm_parts", _P), ("kv_bak", _P),
        ("kv_bak_n", _I64),
        ("epoch", ctypes.c_uint32 * 3), ("tag", ctypes.c_uint32), ("err", ctypes.c_uint32), ("id_out", _I32),
        ("route", _I32 * 8),
    ]


# l3_argmax_part: one (value, index) argmax candidate
ARGMAX_PART = np.dtype([("v", "<f4"), ("i", "<i4")])
ARGMAX_EMPTY = (-np.inf, 0x7FFFFFFF)  # what a lane without a valid column holds
KV_BAK_SLOTS = 32
STORAGES = {"fp32": 0, "bf16": 1, "fp8": 2}


def argmax_parts_sentinel(shape, salt: int = 0) -> np.ndarray:
    """ARGMAX_PART records no kernel writes: finite values and indices, every record different."""
    a = np.empty(shape, ARGMAX_PART)
    a["v"] = gemm_sentinel(shape, 20 + salt)
    a["i"] = (-1000 - np.arange(a.size, dtype=np.int64) - 7919 * salt).astype(np.int32).reshape(shape)
    return a


def int_sentinel(shape, salt: int = 0) -> np.ndarray:
    """Negative int32 ids no kernel writes, every entry different."""
    n = int(np.prod(shape))
    return (-5000 - np.arange(n, dtype=np.int64) - 104729 * salt).astype(np.int32).reshape(shape)


class DecState:
    """A decode state for op_decode_gemm / op_argmax_parts: the description going in, and after the call
    ``pos``, ``arrive`` and the histories ``hist`` (int32) / ``hist_val`` (float32) [hist_cap * rows + 1]
    WITH their guard entry; both start as sentinels (``int_sentinel(n, 3)``, ``gemm_sentinel(n, 11)``)."""

    def __init__(self, pos: int, hist_base: int = 0, hist_cap: int = 0, hist: bool = True, hist_val: bool = True,
                 rows: int = 1, arrive: int = 0):
        self.pos, self.hist_base, self.hist_cap, self.rows, self.arrive = pos, hist_base, hist_cap, rows, arrive
        n = hist_cap * rows + 1
        self.hist = int_sentinel(n, 3) if hist else None
        self.hist_val = gemm_sentinel(n, 11).copy() if hist_val else None

    def _io(self) -> DecStateIO:
        io = DecStateIO()
        io.struct_size = ctypes.sizeof(DecStateIO)
        io.pos, io.hist_base, io.hist_cap, io.arrive = self.pos, self.hist_base, self.hist_cap, self.arrive
        io.hist = ptr(self.hist) if self.hist is not None else None
        io.hist_val = ptr(self.hist_val) if self.hist_val is not None else None
        io.hist_len = self.hist_cap * self.rows + 1
        return io

    def _take(self, io: DecStateIO) -> None:
        self.pos, self.arrive = int(io.pos), int(io.arrive)


def _gemm_route(op) -> dict:
    fam = GEMM_FAMILIES[op.route[0]]
    route = {"family": fam, "launches": int(op.route[6])}
    for i, name in enumerate(_ROUTE_FIELDS[fam]):
        route[name] = int(op.route[1 + i])
    return route


EPI_STORE, EPI_RESID, EPI_SWIGLU, EPI_QKV = range(4)
GEMM_FAMILIES = ["none", "gemv", "gemv_bf16", "skinny", "splitk", "tiled", "x6", "rows_bf16", "gemv_fp8", "rows_fp8"]
_ROUTE_FIELDS = {
    "gemv": ("rows_per_block", "lanes_per_unit", "nt", "row_blocks"),
    "gemv_bf16": ("rows_per_block", "lanes_per_unit", "nt", "row_blocks"),
    "skinny": ("tn", "ch"),
    "splitk": ("bm", "bn", "bk", "s"),
    "tiled": ("bm", "bn", "bk", "stages", "group_m"),
    "x6": ("bm", "bn", "bk", "waves", "group_m"),
    "rows_bf16": ("mt", "waves", "nt", "tn"),
    "gemv_fp8": ("rows_per_block", "lanes_per_unit", "nt", "row_blocks"),
    "rows_fp8": ("mt", "waves", "nt", "tn"),
    "none": (),
}


def gemm_sentinel(shape, salt: int = 0) -> np.ndarray:
    """A NaN-free float32 fill whose every element differs from its neighbours: what op_gemm puts in
    the guard space (and a test in whatever else a launch must not touch), compared bit for bit."""
    n = int(np.prod(shape))
    i = np.arange(n, dtype=np.uint64) + np.uint64(salt) * np.uint64(1000003)
    bits = np.uint32(0x40800000) + ((i * np.uint64(2654435761)) & np.uint64(0x3FFFFF)).astype(np.uint32)
    return bits.view(np.float32).reshape(shape)


ATTN_KERNELS = ["prefill", "decode", "decode_oproj"]  # l3_op_attention_host route[0]


def attn_scale_q(q: np.ndarray, hd: int) -> np.ndarray:
    """q * log2(e) / sqrt(hd) in fp32: the queries as the dense attention kernels take them (the
    QKV epilogue's q_scale), so that p = exp2(q~ . k - max)."""
    return np.asarray(q, np.float32) * np.float32(1.4426950408889634 / np.sqrt(float(hd)))


def interleave_gate_up(wg: np.ndarray, wu: np.ndarray) -> np.ndarray:
    """Separate gate and up [hidden, K] -> the kernels' fused [2 hidden, K] layout (16 gate rows,
    then the 16 up rows of the same hidden units), as l3_op_ffn_host builds it."""
    hidden, K = wg.shape
    if wu.shape != wg.shape or hidden % 16:
        raise ValueError(f"gate {wg.shape} and up {wu.shape} must be equal with hidden % 16 == 0")
    return np.ascontiguousarray(np.stack([wg.reshape(hidden // 16, 16, K), wu.reshape(hidden // 16, 16, K)],
                                         axis=1).reshape(2 * hidden, K))

_lib: Optional[ctypes.CDLL] = None


def lib() -> ctypes.CDLL:
    """Load the HIP library (built by ``__graft_entry__.build()`` / ``make -C csrc``)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"libllama3hip.so not found at {LIB_PATH}: build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` (no CPU fallback exists)")
        so = ctypes.CDLL(LIB_PATH)
        other = bool(os.environ.get("L3_LIB_PATH"))  # an older A/B build may lack newer entry points
        for name, (res, args) in _SIGNATURES.items():
            if other and not hasattr(so, name):
                continue
            fn = getattr(so, name)
            fn.restype = res
            fn.argtypes = args
        _lib = so
    return _lib


def header_symbols() -> List[str]:
    """Every function the public header declares (used by the ABI test)."""
    with open(HEADER) as f:
        text = f.read()
    return sorted(set(re.findall(r"^(?:int|const char\*)\s+(l3_\w+)\s*\(", text, re.M)))


def check(rc: int) -> None:
    if rc != 0:
        raise RuntimeError("libllama3hip: " + lib().l3_last_error().decode(errors="replace"))


def ptr(a: np.ndarray) -> int:
    return a.ctypes.data


def version() -> str:
    """Library version; bumped whenever a hot kernel changes (keys profile artifacts)."""
    major, minor = ctypes.c_int32(0), ctypes.c_int32(0)
    check(lib().l3_version(ctypes.byref(major), ctypes.byref(minor)))
    return f"{major.value}.{minor.value}"


def source_hash() -> str:
    """sha256 prefix of the sources the loaded library was built from (keys profiles)."""
    return lib().l3_source_hash().decode()


class PinnedPool:
    """Page-locked host buffers handed out as NumPy arrays (``l3_host_alloc``).

    The library's host-path copies (logits D2H of ``Llama.__call__``) run as DMA at PCIe
    rate into such a buffer instead of through a pageable bounce.  The array owns its
    block through a ctypes buffer object; once the array and every view of it are gone the
    block returns to a free list and the next call of the same size reuses it (at most
    ``keep`` free blocks are kept, the rest are freed).

    Bounded: at most ``max_bytes`` are page-locked at once (blocks handed out plus cached); a
    request beyond that, or smaller than ``min_bytes`` (where pinning buys nothing), gets an
    ordinary ``np.empty`` array instead, so a caller that keeps many results never pins
    unbounded host memory."""

    def __init__(self, keep: int = 4, max_bytes: int = 1 << 30, min_bytes: int = 1 << 16):
        import threading

        self.keep = keep
        self.max_bytes = max_bytes
        self.min_bytes = min_bytes
        self._free = {}  # nbytes -> [address]
        self._pinned = 0  # bytes page-locked now: handed out + cached
        self._lock = threading.Lock()

    def empty(self, shape, dtype) -> np.ndarray:
        import weakref

        dtype = np.dtype(dtype)
        n = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
        nb = max(n, 64)
        if nb < self.min_bytes:
            return np.empty(shape, dtype)
        with self._lock:
            blocks = self._free.get(nb)
            addr = blocks.pop() if blocks else None
            if addr is None:
                if self._pinned + nb > self.max_bytes:
                    return np.empty(shape, dtype)
                self._pinned += nb  # reserved before the allocation
        if addr is None:
            p = ctypes.c_void_p()
            try:
                check(lib().l3_host_alloc(nb, ctypes.byref(p)))
            except Exception:
                with self._lock:
                    self._pinned -= nb
                raise
            addr = p.value
        holder = (ctypes.c_char * nb).from_address(addr)
        weakref.finalize(holder, self._release, addr, nb)
        return np.frombuffer(holder, dtype=dtype, count=n // dtype.itemsize).reshape(shape)

    def _release(self, addr: int, nb: int) -> None:
        with self._lock:
            blocks = self._free.setdefault(nb, [])
            if len(blocks) < self.keep:
                blocks.append(addr)
                return
            self._pinned -= nb
        lib().l3_host_free(addr)

    @property
    def pinned_bytes(self) -> int:
        return self._pinned

    def clear(self) -> None:
        """Free every cached block (arrays still alive are freed when dropped)."""
        with self._lock:
            blocks = [(a, nb) for nb, v in self._free.items() for a in v]
            self._free.clear()
            self.keep = 0
            self._pinned -= sum(nb for _, nb in blocks)
        for addr, _ in blocks:
            lib().l3_host_free(addr)


pinned = PinnedPool()


def sample_uniform(seed: int, row: int, pos: int) -> float:
    """The uniform in [0, 1) a sampling step draws for (seed, batch row, position): Philox4x32-10,
    (x0 >> 8) * 2^-24 (l3_sample_uniform; host only, no device)."""
    u = ctypes.c_float(0.0)
    check(lib().l3_sample_uniform(int(seed) & (2 ** 64 - 1), int(row), int(pos), ctypes.byref(u)))
    return float(u.value)


def device_count() -> int:
    n = ctypes.c_int32(0)
    check(lib().l3_device_count(ctypes.byref(n)))
    return n.value


# KV-cache storage types (enum l3_kv_dtype) by the name ``Context(..., kv_dtype=...)`` takes
KV_DTYPES = {None: 0, "bf16": 1}


def kv_dtype_code(kv_dtype) -> int:
    """The ``l3_kv_dtype`` code of ``kv_dtype`` (None: fp32, "bf16"); ValueError for anything else."""
    if not (kv_dtype is None or isinstance(kv_dtype, str)) or kv_dtype not in KV_DTYPES:
        raise ValueError(f"kv_dtype {kv_dtype!r}: None (fp32) or 'bf16'")
    return KV_DTYPES[kv_dtype]


def _kv_caches(cache_k, cache_v):
    """Contiguous copies of an op's caches and their l3_kv_dtype code: uint16 arrays are bf16 bit
    patterns, anything else is taken as fp32."""
    bf = np.asarray(cache_k).dtype == np.uint16
    if bf != (np.asarray(cache_v).dtype == np.uint16):
        raise ValueError("cache_k and cache_v must both be uint16 (bf16 bits) or both fp32")
    dt = np.uint16 if bf else np.float32
    return np.array(cache_k, dtype=dt, order="C"), np.array(cache_v, dtype=dt, order="C"), int(bf)


class Context:
    """Owns one device context (weights, KV caches, workspace) on one GPU.  ``kv_dtype`` (extension;
    DESIGN.md "bf16 KV-cache storage"): None, the fp32 caches; "bf16", caches of two bytes per
    element that only the ragged entry points serve (l3_create_kv)."""

    def __init__(self, dims: Dims, device: int = 0, kv_dtype=None):
        code = kv_dtype_code(kv_dtype)
        self._h = ctypes.c_void_p()
        if code:
            check(lib().l3_create_kv(device, ctypes.byref(dims), code, ctypes.byref(self._h)))
        else:
            check(lib().l3_create(device, ctypes.byref(dims), ctypes.byref(self._h)))
        self.kv_dtype = kv_dtype
        self.dims = dims
        self.device = device
        self._owned = True

    @classmethod
    def _member(cls, handle: ctypes.c_void_p, dims: Dims, device: int, group) -> "Context":
        """A group member's context: owned by the group (never destroyed through this object,
        which keeps the group alive)."""
        c = cls.__new__(cls)
        c._h, c.dims, c.device, c._owned, c._group = handle, dims, device, False, group
        c.kv_dtype = None  # a group's members are fp32 contexts
        return c

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h and getattr(self, "_owned", True):
            lib().l3_destroy(self._h)
        self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- weights ----
    def upload(self, layer: int, kind: int, w: np.ndarray) -> None:
        a = np.ascontiguousarray(w, dtype=np.float32)
        rows, cols = (1, a.shape[0]) if a.ndim == 1 else a.shape
        check(lib().l3_upload_weight(self._h, layer, kind, ptr(a), rows, cols))

    def finalize(self) -> None:
        check(lib().l3_finalize(self._h))

    def reset_cache(self) -> None:
        check(lib().l3_reset_cache(self._h))

    def kv_info(self) -> dict:
        """The KV-cache storage type (None or "bf16") and the bytes of all layers' K and V
        allocations (l3_kv_info)."""
        dt, n = ctypes.c_int32(0), ctypes.c_int64(0)
        check(lib().l3_kv_info(self._h, ctypes.byref(dt), ctypes.byref(n)))
        return {"dtype": {v: k for k, v in KV_DTYPES.items()}[dt.value], "bytes": n.value}

    def cache_read(self, layer: int, row: int, slot0: int, n: int):
        """Slots ``[slot0, slot0 + n)`` of cache row ``row`` of one layer (l3_cache_read_host):
        (k, v), each [n_kv_heads, n, head_dim] fp32 — a bf16 cache's values widened exactly."""
        shape = (self.dims.n_kv_heads, max(int(n), 0), self.dims.dim // self.dims.n_heads)
        k, v = np.empty(shape, np.float32), np.empty(shape, np.float32)
        check(lib().l3_cache_read_host(self._h, int(layer), int(row), int(slot0), int(n), ptr(k), ptr(v)))
        return k, v

    # ---- forward ----
    def forward(self, ids: np.ndarray, start_pos: int) -> np.ndarray:
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        B, L = ids.shape
        out = pinned.empty((B, self.dims.vocab_size), np.float32)  # DMA target of the D2H
        check(lib().l3_forward_host(self._h, ptr(ids), B, L, start_pos, ptr(out)))
        return out

    def score(self, ids: np.ndarray, targets: np.ndarray, start_pos: int, want_argmax: bool = False):
        """Teacher-forced scoring (l3_score_host): one forward over ``ids`` [B, L] that returns
        float32 [B, L] with the log-probability of ``targets`` [B, L] at every position (-1: no
        target, scored 0.0), without materialising the logits; with ``want_argmax`` also the int32
        greedy id of every position.  Writes the K / V cache as ``forward`` does."""
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        targets = np.ascontiguousarray(targets, dtype=np.int64)
        if ids.ndim != 2 or targets.shape != ids.shape:
            raise ValueError(f"ids {ids.shape} and targets {targets.shape} must be the same [B, L]")
        B, L = ids.shape
        lp = np.empty((B, L), np.float32)
        am = np.empty((B, L), np.int32) if want_argmax else None
        check(lib().l3_score_host(self._h, ptr(ids), ptr(targets), B, L, int(start_pos), ptr(lp),
                                  ptr(am) if am is not None else None))
        return (lp, am) if want_argmax else lp

    def set_score_workspace(self, nbytes: int) -> None:
        """Bytes of the scoring workspace (16 per row and 64 columns of the vocabulary; default
        64 MiB, 0 restores it).  The scores do not depend on it, bit for bit."""
        check(lib().l3_set_score_workspace(self._h, int(nbytes)))

    def greedy_step(self, ids: np.ndarray, start_pos: int, want_logits: bool = False):
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        B, L = ids.shape
        nxt = np.empty(B, np.int64)
        logits = pinned.empty((B, self.dims.vocab_size), np.float32) if want_logits else None
        check(lib().l3_greedy_step_host(self._h, ptr(ids), B, L, start_pos, ptr(nxt),
                                        ptr(logits) if logits is not None else None))
        return nxt, logits

    def set_sampling(self, temperature: float = 0.0, top_k: int = 0, top_p: float = 1.0, seed: int = 0) -> None:
        """Temperature / top-k / top-p sampling for ``greedy_step`` / ``greedy_generate``
        (l3_set_sampling); temperature 0 restores greedy decoding.  Each token's uniform is a
        function of (seed, batch row, position), so one seed gives one sequence on every path."""
        check(lib().l3_set_sampling(self._h, float(temperature), int(top_k), float(top_p),
                                    int(seed) & (2 ** 64 - 1)))

    def get_sampling(self) -> dict:
        t, k, p, s = ctypes.c_float(0), ctypes.c_int32(0), ctypes.c_float(0), ctypes.c_uint64(0)
        check(lib().l3_get_sampling(self._h, ctypes.byref(t), ctypes.byref(k), ctypes.byref(p), ctypes.byref(s)))
        return {"temperature": t.value, "top_k": k.value, "top_p": p.value, "seed": s.value}

    def greedy_generate(self, ids: np.ndarray, max_new_tokens: int, values: bool = False):
        """The device-side greedy loop: ids [B, max_new_tokens - L]; with ``values`` also each
        step's winning logit (fp32, same shape) — the value the step's argmax picked.  With
        sampling on (``set_sampling``) the ids are sampled and the value is the picked token's."""
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        B, L = ids.shape
        out = np.empty((B, max(0, max_new_tokens - L)), np.int64)
        if not values:
            check(lib().l3_greedy_generate_host(self._h, ptr(ids), B, L, max_new_tokens, ptr(out)))
            return out
        vals = np.empty(out.shape, np.float32)
        check(lib().l3_greedy_generate_values_host(self._h, ptr(ids), B, L, max_new_tokens, ptr(out), ptr(vals)))
        return out, vals

    @staticmethod
    def _ragged_args(ids, lens):
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        if ids.ndim != 2 or lens.shape != (ids.shape[0],):
            raise ValueError(f"ids {ids.shape} must be [B, Lmax] and lens {lens.shape} [B]")
        return ids, lens

    def ragged_forward(self, ids: np.ndarray, lens) -> np.ndarray:
        """Prefill of prompts of different lengths (l3_ragged_forward_host): ``ids`` [B, Lmax]
        right-padded (pad entries are ignored), ``lens`` [B]; float32 [B, VS], row b the logits of
        its position ``lens[b] - 1``.  Leaves slots ``[lens[b], Lmax)`` of cache row b zero."""
        ids, lens = self._ragged_args(ids, lens)
        B, Lmax = ids.shape
        out = pinned.empty((B, self.dims.vocab_size), np.float32)
        check(lib().l3_ragged_forward_host(self._h, ptr(ids), ptr(lens), B, Lmax, ptr(out)))
        return out

    @staticmethod
    def _ragged_starts(starts, B):
        starts = np.ascontiguousarray(starts, dtype=np.int32)
        if starts.shape != (B,):
            raise ValueError(f"starts {starts.shape} must be [{B}]")
        return starts

    def ragged_extend(self, ids: np.ndarray, lens, starts) -> np.ndarray:
        """Several new tokens per row, each row at its own offset (l3_ragged_extend_host): row b's
        ``lens[b]`` tokens of ``ids`` [B, Lmax] (right-padded, pads ignored) run at positions
        ``[starts[b], starts[b] + lens[b])`` over the row's cache as it stands; float32 [B, VS],
        row b the logits of its last new token.  No other cache slot changes."""
        ids, lens = self._ragged_args(ids, lens)
        B, Lmax = ids.shape
        starts = self._ragged_starts(starts, B)
        out = pinned.empty((B, self.dims.vocab_size), np.float32)
        check(lib().l3_ragged_extend_host(self._h, ptr(ids), ptr(lens), ptr(starts), B, Lmax, ptr(out)))
        return out

    def ragged_generate(self, ids: np.ndarray, lens, max_new_tokens: int, stop_ids=(), starts=None):
        """The device-side decode loop over rows of different lengths (l3_ragged_generate_host):
        (out int64 [B, max_new_tokens - min(lens)], out_lens int32 [B]); row b holds
        ``out_lens[b]`` tokens — at most ``max_new_tokens - lens[b]``, fewer when it emitted one of
        ``stop_ids`` (kept as its last token) — and -1 after them.  Sampled when ``set_sampling``
        is on, with the uniforms of (seed, row, position).  With ``starts`` [B]
        (l3_ragged_generate_from_host) the rows continue from their caches: ``ids`` run at
        ``starts[b]`` on, and ``starts[b] + lens[b]`` stands in the length's place everywhere.
        When no row of the batch has a token to emit (``max_new_tokens <= starts[b] + lens[b]`` for
        every b) the call runs nothing, as without ``starts``: the new tokens are NOT appended to
        the caches then — use ``ragged_extend`` to append without generating."""
        ids, lens = self._ragged_args(ids, lens)
        B, Lmax = ids.shape
        stops = np.ascontiguousarray(list(stop_ids), dtype=np.int64).reshape(-1)
        if starts is not None:
            starts = self._ragged_starts(starts, B)
        total = lens if starts is None else lens.astype(np.int64) + starts
        cap = max(0, int(max_new_tokens) - int(total.min())) if B else 0
        out = np.full((B, cap), -1, np.int64)
        out_lens = np.zeros(B, np.int32)
        tail = (B, Lmax, int(max_new_tokens), ptr(stops) if stops.size else None, int(stops.size), ptr(out),
                ptr(out_lens))
        if starts is None:
            check(lib().l3_ragged_generate_host(self._h, ptr(ids), ptr(lens), *tail))
        else:
            check(lib().l3_ragged_generate_from_host(self._h, ptr(ids), ptr(lens), ptr(starts), *tail))
        return out, out_lens

    def ragged_generate_spec(self, ids: np.ndarray, lens, max_new_tokens: int, stop_ids=(), starts=None,
                             lookup=None, lookup_lens=None, draft_len: int = 4, ngram_max: int = 3,
                             ngram_min: int = 1):
        """``ragged_generate`` through speculative iterations with lookup drafts
        (l3_ragged_generate_spec_host): the same (out, out_lens), and a dict of per-row int32
        counters — ``row_steps`` (iterations in which the row ran a chunk), ``drafted`` and
        ``accepted`` (draft tokens run / confirmed).  ``lookup`` int64 [B, Lk] with ``lookup_lens``
        [B] is an optional reference text per row that the n-gram lookup searches before the row's
        own tokens."""
        ids, lens = self._ragged_args(ids, lens)
        B, Lmax = ids.shape
        stops = np.ascontiguousarray(list(stop_ids), dtype=np.int64).reshape(-1)
        if starts is not None:
            starts = self._ragged_starts(starts, B)
        if lookup is not None:
            lookup = np.ascontiguousarray(lookup, dtype=np.int64)
            lookup_lens = np.ascontiguousarray(lookup_lens, dtype=np.int32)
            if lookup.ndim != 2 or lookup.shape[0] != B or lookup_lens.shape != (B,):
                raise ValueError(f"lookup {lookup.shape} must be [{B}, Lk] and lookup_lens {lookup_lens.shape} [{B}]")
        total = lens if starts is None else lens.astype(np.int64) + starts
        cap = max(0, int(max_new_tokens) - int(total.min())) if B else 0
        out = np.full((B, cap), -1, np.int64)
        out_lens = np.zeros(B, np.int32)
        stats = {k: np.zeros(B, np.int32) for k in ("row_steps", "drafted", "accepted")}
        check(lib().l3_ragged_generate_spec_host(
            self._h, ptr(ids), ptr(lens), None if starts is None else ptr(starts), B, Lmax, int(max_new_tokens),
            ptr(stops) if stops.size else None, int(stops.size),
            None if lookup is None else ptr(lookup), None if lookup is None else ptr(lookup_lens),
            0 if lookup is None else lookup.shape[1], int(draft_len), int(ngram_max), int(ngram_min),
            ptr(out), ptr(out_lens), ptr(stats["row_steps"]), ptr(stats["drafted"]), ptr(stats["accepted"])))
        return out, out_lens, stats

    def ragged_verify(self, ids: np.ndarray, lens, starts):
        """An extend that returns the model's token choice at every chunk position
        (l3_ragged_verify_host): (chosen int64 [B, Lmax], -1 at pads; n_accept int32 [B], the
        length of the prefix of ``ids[b][1:]`` that equals those choices).  The cache effect is
        ``ragged_extend``'s."""
        ids, lens = self._ragged_args(ids, lens)
        B, Lmax = ids.shape
        starts = self._ragged_starts(starts, B)
        chosen = np.full((B, Lmax), -1, np.int64)
        n_accept = np.zeros(B, np.int32)
        check(lib().l3_ragged_verify_host(self._h, ptr(ids), ptr(lens), ptr(starts), B, Lmax, ptr(chosen),
                                          ptr(n_accept)))
        return chosen, n_accept

    def op_spec_draft(self, seq, seq_lens, k, draft_len: int, ngram_max: int = 3, ngram_min: int = 1):
        """The lookup drafting rule on plain arrays (l3_op_spec_draft_host): ``seq`` int32
        [B, Smax], ``seq_lens`` / ``k`` [B]; returns (out int32 [B, draft_len], -1 past each
        draft; out_n int32 [B])."""
        seq = np.ascontiguousarray(seq, dtype=np.int32)
        seq_lens = np.ascontiguousarray(seq_lens, dtype=np.int32)
        k = np.ascontiguousarray(k, dtype=np.int32)
        if seq.ndim != 2 or seq_lens.shape != (seq.shape[0],) or k.shape != seq_lens.shape:
            raise ValueError(f"seq {seq.shape} must be [B, Smax], seq_lens {seq_lens.shape} and k {k.shape} [B]")
        B, Smax = seq.shape
        out = np.full((B, int(draft_len)), -1, np.int32)
        out_n = np.zeros(B, np.int32)
        check(lib().l3_op_spec_draft_host(self._h, ptr(seq), ptr(seq_lens), ptr(k), B, Smax, int(draft_len),
                                          int(ngram_max), int(ngram_min), ptr(out) if out.size else None,
                                          ptr(out_n)))
        return out, out_n

    def cache_copy_rows(self, src: int, dst_rows, n_slots: int) -> None:
        """The fork of a cache row (l3_cache_copy_rows): slots ``[0, n_slots)`` of K and V in every
        layer from row ``src`` to each row of ``dst_rows``."""
        dst = np.ascontiguousarray(list(dst_rows), dtype=np.int32).reshape(-1)
        check(lib().l3_cache_copy_rows(self._h, int(src), ptr(dst) if dst.size else None, int(dst.size), int(n_slots)))

    def op_attn_extend_ragged(self, qkv, cache_k, cache_v, rope_cos, rope_sin, starts, lens, n_heads: int):
        """The two launches of a ragged extend on plain arrays (l3_op_attn_extend_ragged_host):
        ``qkv`` [B, Lq, (H + 2 KVH) * HD] raw rows, ``cache_k`` / ``cache_v`` [B, KVH, Smax, HD],
        ``rope_cos`` / ``rope_sin`` [Smax, HD/2], ``starts`` / ``lens`` [B].  Returns
        (out [B, Lq, H * HD], cache_k, cache_v) — the caches are copies with slots
        ``[starts[b], starts[b] + lens[b])`` written.  uint16 caches are bf16 bit patterns
        (l3_op_attn_extend_ragged_kv_host): the new K / V are rounded as they are stored."""
        ck, cv, kv = _kv_caches(cache_k, cache_v)
        if ck.ndim != 4 or cv.shape != ck.shape:
            raise ValueError(f"cache_k {ck.shape} / cache_v {cv.shape} must be [B, KVH, Smax, HD]")
        B, KVH, Smax, HD = ck.shape
        H = int(n_heads)
        qkv = np.ascontiguousarray(qkv, dtype=np.float32)
        c = np.ascontiguousarray(rope_cos, dtype=np.float32)
        s = np.ascontiguousarray(rope_sin, dtype=np.float32)
        starts = np.ascontiguousarray(starts, dtype=np.int32)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        if qkv.ndim != 3 or qkv.shape[0] != B or qkv.shape[2] != (H + 2 * KVH) * HD or c.shape != (Smax, HD // 2) \
                or s.shape != c.shape:
            raise ValueError(f"qkv {qkv.shape} / rope tables {c.shape} do not match the caches {ck.shape}")
        if starts.shape != (B,) or lens.shape != (B,):
            raise ValueError(f"starts {starts.shape} and lens {lens.shape} must be [{B}]")
        Lq = qkv.shape[1]
        out = np.empty((B, Lq, H * HD), np.float32)
        if kv:
            check(lib().l3_op_attn_extend_ragged_kv_host(self._h, ptr(qkv), ptr(ck), ptr(cv), kv, ptr(c), ptr(s),
                                                         ptr(starts), ptr(lens), B, Lq, H, KVH, HD, Smax, ptr(out)))
            return out, ck, cv
        check(lib().l3_op_attn_extend_ragged_host(self._h, ptr(qkv), ptr(ck), ptr(cv), ptr(c), ptr(s), ptr(starts),
                                                  ptr(lens), B, Lq, H, KVH, HD, Smax, ptr(out)))
        return out, ck, cv

    def set_ragged_attn_split(self, mode: int, chunk: int = 0) -> None:
        """Extension (l3_set_ragged_attn_split): the split-KV decode attention of the ragged
        decode step — ``mode`` 0 auto (only where the single-pass kernel's LDS does not fit; the
        default), 1 always; ``chunk`` keys per chunk, a multiple of 64 in [64, 4096] (0 keeps the
        current one)."""
        check(lib().l3_set_ragged_attn_split(self._h, int(mode), int(chunk)))

    def ragged_attn_info(self) -> dict:
        """The split mode, the chunk length in force, the attention launches served by the split
        form and the bytes of its workspace."""
        m, ch, n, b = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_int64(0)
        check(lib().l3_ragged_attn_info(self._h, ctypes.byref(m), ctypes.byref(ch), ctypes.byref(n), ctypes.byref(b)))
        return {"mode": m.value, "chunk": ch.value, "split_launches": n.value, "workspace_bytes": b.value}

    def op_attn_decode_ragged(self, qkv, cache_k, cache_v, rope_cos, rope_sin, pos, finished, n_heads: int,
                              s_cap: int, split: int = 0):
        """One ragged decode-attention launch on plain arrays (l3_op_attn_decode_ragged_host):
        ``qkv`` [B, (H + 2 KVH) * HD] raw rows, ``cache_k`` / ``cache_v`` [B, KVH, Smax, HD],
        ``rope_cos`` / ``rope_sin`` [Smax, HD/2], ``pos`` / ``finished`` [B]; ``split`` 0 runs the
        single-pass kernel, else the split-KV form at that chunk length.  Returns
        (out [B, H * HD], cache_k, cache_v) — the caches are copies with slot ``pos[b]`` appended.
        uint16 caches are bf16 bit patterns (l3_op_attn_decode_ragged_kv_host): the new k / v are
        rounded as they are stored, and used as rounded."""
        ck, cv, kv = _kv_caches(cache_k, cache_v)
        if ck.ndim != 4 or cv.shape != ck.shape:
            raise ValueError(f"cache_k {ck.shape} / cache_v {cv.shape} must be [B, KVH, Smax, HD]")
        B, KVH, Smax, HD = ck.shape
        H = int(n_heads)
        qkv = np.ascontiguousarray(qkv, dtype=np.float32)
        c = np.ascontiguousarray(rope_cos, dtype=np.float32)
        s = np.ascontiguousarray(rope_sin, dtype=np.float32)
        pos = np.ascontiguousarray(pos, dtype=np.int32)
        fin = np.ascontiguousarray(finished, dtype=np.int32)
        if qkv.shape != (B, (H + 2 * KVH) * HD) or c.shape != (Smax, HD // 2) or s.shape != c.shape:
            raise ValueError(f"qkv {qkv.shape} / rope tables {c.shape} do not match the caches {ck.shape}")
        if pos.shape != (B,) or fin.shape != (B,):
            raise ValueError(f"pos {pos.shape} and finished {fin.shape} must be [{B}]")
        out = np.empty((B, H * HD), np.float32)
        if kv:
            check(lib().l3_op_attn_decode_ragged_kv_host(self._h, ptr(qkv), ptr(ck), ptr(cv), kv, ptr(c), ptr(s),
                                                         ptr(pos), ptr(fin), B, H, KVH, HD, Smax, int(s_cap), int(split),
                                                         ptr(out)))
            return out, ck, cv
        check(lib().l3_op_attn_decode_ragged_host(self._h, ptr(qkv), ptr(ck), ptr(cv), ptr(c), ptr(s), ptr(pos),
                                                  ptr(fin), B, H, KVH, HD, Smax, int(s_cap), int(split), ptr(out)))
        return out, ck, cv

    def layer_forward(self, layer: int, x: np.ndarray, start_pos: int) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.float32)
        B, L, _ = x.shape
        out = np.empty_like(x)
        check(lib().l3_layer_forward_host(self._h, layer, ptr(x), B, L, start_pos, ptr(out)))
        return out

    def attention_forward(self, layer: int, x: np.ndarray, start_pos: int) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.float32)
        B, L, _ = x.shape
        out = np.empty_like(x)
        check(lib().l3_attention_forward_host(self._h, layer, ptr(x), B, L, start_pos, ptr(out)))
        return out

    # ---- device buffers (bench) ----
    def alloc(self, nbytes: int) -> int:
        p = ctypes.c_void_p()
        check(lib().l3_dev_alloc(self._h, nbytes, ctypes.byref(p)))
        return p.value

    def free(self, p: int) -> None:
        check(lib().l3_dev_free(self._h, p))

    def h2d(self, dst: int, a: np.ndarray) -> None:
        a = np.ascontiguousarray(a)
        check(lib().l3_h2d(self._h, dst, ptr(a), a.nbytes))

    def d2h(self, a: np.ndarray, src: int) -> np.ndarray:
        check(lib().l3_d2h(self._h, ptr(a), src, a.nbytes))
        return a

    def forward_dev(self, ids_dev: int, B: int, L: int, start_pos: int, logits_dev: int) -> None:
        check(lib().l3_forward_dev(self._h, ids_dev, B, L, start_pos, logits_dev))

    def set_batch_split(self, parts: int, min_tokens: int = 8192) -> None:
        """Run a model forward as `parts` batch-row ranges on their own streams (extension;
        results bit-identical for any split, default 2)."""
        check(lib().l3_set_batch_split(self._h, int(parts), int(min_tokens)))

    def set_last_layer_rows(self, all_rows: bool) -> None:
        """Extension: False (default) runs the last block's attention / O-proj / FFN on each
        sequence's last position only (l3_set_last_layer_rows); True, every position."""
        check(lib().l3_set_last_layer_rows(self._h, int(bool(all_rows))))

    def set_gemm_x6(self, on: bool) -> None:
        """Extension (l3_set_gemm_x6): the prefill projections on the x6 kernel — fp32 operands
        cut exactly into three bf16 pieces, six bf16 MFMA products per fp32 product (error
        against fp64 at or below the fp32 MFMA kernel's); off (default) frees the pieces."""
        check(lib().l3_set_gemm_x6(self._h, int(bool(on))))

    def set_embed_qkv(self, on: bool, max_bytes: int = 0) -> None:
        """Extension (l3_set_embed_qkv): layer 0's QKV of a prefill past 256 rows as a lookup in a
        table of its pre-RoPE rows per token id (bit-identical to the GEMM; on by default).  The
        table is built at first use if it fits max_bytes (0 keeps the limit, 256 MB by default)."""
        check(lib().l3_set_embed_qkv(self._h, int(bool(on)), int(max_bytes)))

    def set_ffn_fused(self, on: bool) -> None:
        """Extension (l3_set_ffn_fused): gate|up + down of a block past 256 rows (dim 288, fp32
        weights) as one launch that keeps the hidden activations in registers (bit-identical to
        the two GEMMs; on by default)."""
        check(lib().l3_set_ffn_fused(self._h, int(bool(on))))

    def set_weight_bf16(self, mode: int) -> None:
        """Extension (l3_set_weight_bf16): bf16 storage of the projections and the lm_head for the
        weight-streaming decode GEMVs — 0 off, 1 exact (every element must be a bf16 value, else
        ``finalize`` fails), 2 round (the weights are rounded).  Before ``finalize`` only."""
        check(lib().l3_set_weight_bf16(self._h, int(mode)))

    def weight_bf16_info(self) -> dict:
        """The mode, the bytes of the bf16 copies and the GEMV launches issued on them."""
        m, b, n = ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_int64(0)
        check(lib().l3_weight_bf16_info(self._h, ctypes.byref(m), ctypes.byref(b), ctypes.byref(n)))
        return {"mode": m.value, "bytes": b.value, "gemv_launches": n.value}

    def set_weight_fp8(self, mode: int) -> None:
        """Extension (l3_set_weight_fp8): per-row power-of-two scaled fp8 e4m3 storage of the
        projections and the lm_head for the 1 .. 64-row decode kernels — 0 off, 1 exact (every
        element must equal ``utils.round_fp8_rows`` of itself, else ``finalize`` raises naming the
        tensor), 2 round (the fp32 weights become those values too).  Before ``finalize``; not
        together with ``set_weight_bf16``."""
        check(lib().l3_set_weight_fp8(self._h, int(mode)))

    def weight_fp8_info(self) -> dict:
        """The mode, the bytes of the code and scale copies, and the launches issued on them by the
        GEMV's fp8 form and by the rows kernel's."""
        m, b, n, r = ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        check(lib().l3_weight_fp8_info(self._h, ctypes.byref(m), ctypes.byref(b), ctypes.byref(n), ctypes.byref(r)))
        return {"mode": int(m.value), "bytes": int(b.value), "gemv_launches": int(n.value),
                "rows_launches": int(r.value)}

    def set_weight_bf16_rows(self, max_rows: Optional[int] = None, min_bytes: Optional[int] = None) -> None:
        """Extension (l3_set_weight_bf16_rows): with bf16 weight storage on, launches of 2 ..
        ``max_rows`` rows (0: off; at most 64) against a weight of at least ``min_bytes`` bf16 bytes
        run on the weight-streaming MFMA kernel that reads the bf16 copy once.  ``None`` keeps a
        value.  Before or after ``finalize``; a change re-captures the decode steps."""
        check(lib().l3_set_weight_bf16_rows(self._h, -1 if max_rows is None else int(max_rows),
                                            -1 if min_bytes is None else int(min_bytes)))

    def weight_bf16_rows_info(self) -> dict:
        """``max_rows`` and ``min_bytes`` in force and the ``launches`` issued on that kernel."""
        r, b, n = ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_int64(0)
        check(lib().l3_weight_bf16_rows_info(self._h, ctypes.byref(r), ctypes.byref(b), ctypes.byref(n)))
        return {"max_rows": r.value, "min_bytes": b.value, "launches": n.value}

    def synchronize(self) -> None:
        check(lib().l3_synchronize(self._h))

    def kernel_timing(self, enable, kernels=None) -> None:
        """Record HIP events around launches (all kernels, or only the named ones)."""
        mask = 0
        if enable:
            names = KERNELS if kernels is None else kernels
            for k in names:
                mask |= 1 << KERNELS.index(k)
        check(lib().l3_kernel_timing(self._h, mask))

    def kernel_stats(self) -> dict:
        ms = np.zeros(len(KERNELS), np.float64)
        cnt = np.zeros(len(KERNELS), np.int64)
        check(lib().l3_kernel_stats(self._h, ptr(ms), ptr(cnt)))
        return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(KERNELS)}

    def set_decode_horizon(self, end_pos: int) -> None:
        """Lazy decode runs ahead of the caller on the device; never at positions >= end_pos."""
        check(lib().l3_set_decode_horizon(self._h, int(end_pos)))

    def decode_persistent(self) -> bool:
        """True when the captured batch-1 decode step is the persistent one-launch kernel."""
        v = ctypes.c_int32(0)
        check(lib().l3_decode_persistent(self._h, ctypes.byref(v)))
        return bool(v.value)

    def decode_recoveries(self) -> int:
        """Persistent decode steps that gave up on a hand-off and were re-run on the graph path."""
        v = ctypes.c_int64(0)
        check(lib().l3_decode_recoveries(self._h, ctypes.byref(v)))
        return int(v.value)

    def device_check_counts(self):
        """(enabled, counts): the device bounds-check counters (check build, L3_LIB_PATH =
        libllama3hip_check.so) since the last call — K / V slot, attention keys, token id."""
        n = np.zeros(4, np.uint32)
        en = ctypes.c_int32(0)
        check(lib().l3_device_check_counts(self._h, n.ctypes.data_as(ctypes.c_void_p), ctypes.byref(en)))
        return bool(en.value), {"kv_slot": int(n[0]), "attn_keys": int(n[1]), "token_id": int(n[2])}

    def device_check_selftest(self) -> None:
        """One recorded violation of each check class (check build; a no-op in the release one)."""
        check(lib().l3_device_check_selftest(self._h))

    def decode_stats(self) -> dict:
        """Decode steps served by graph replay, and of those by a speculative step."""
        v = np.zeros(2, np.int64)
        check(lib().l3_decode_stats(self._h, ptr(v[0:1]), ptr(v[1:2])))
        return {"graph_steps": int(v[0]), "speculative_hits": int(v[1])}

    # ---- RCCL ----
    def comm_init(self, nranks: int, rank: int, uid: bytes) -> None:
        buf = (ctypes.c_uint8 * 128).from_buffer_copy(uid)
        check(lib().l3_comm_init(self._h, nranks, rank, buf))
        self.nranks, self.rank = nranks, rank

    def _rows(self, rows_per_rank) -> np.ndarray:
        rows = np.ascontiguousarray(rows_per_rank, dtype=np.int64)
        n = getattr(self, "nranks", None)
        if n is None:
            raise RuntimeError("communicator not initialised (comm_init)")
        if rows.shape != (n,):
            raise ValueError(f"rows_per_rank has {rows.size} entries, the communicator {n} ranks")
        return rows

    def gather_logits(self, src_dev: int, dst_dev: Optional[int], rows_per_rank, root: int = 0):
        rows = self._rows(rows_per_rank)
        check(lib().l3_comm_gather_logits(self._h, src_dev, dst_dev or 0, ptr(rows), root))

    def gather_argmax(self, src_dev: int, dst_dev: Optional[int], rows_per_rank, root: int = 0):
        """Greedy ids only: each rank's argmax over its logits rows, int32 ids gathered to
        ``dst_dev`` [sum rows] on the root (SURVEY 8(e) option)."""
        rows = self._rows(rows_per_rank)
        check(lib().l3_comm_gather_argmax(self._h, src_dev, dst_dev or 0, ptr(rows), root))

    def comm_info(self, gather_busids: bool = True) -> dict:
        """What RCCL reports for this rank (ncclCommCount / ncclCommUserRank /
        ncclCommCuDevice) and, with ``gather_busids`` (collective: every rank calls it), every
        rank's PCI bus id in rank order."""
        n, r, d = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
        cap = getattr(self, "nranks", 1) if gather_busids else 0
        buf = ctypes.create_string_buffer(BUSID_LEN * max(cap, 1))
        check(lib().l3_comm_info(self._h, ctypes.byref(n), ctypes.byref(r), ctypes.byref(d),
                                 buf if gather_busids else None, cap))
        out = {"nranks": n.value, "rank": r.value, "device": d.value}
        if gather_busids:
            raw = buf.raw
            out["busids"] = [raw[i * BUSID_LEN:(i + 1) * BUSID_LEN].split(b"\0")[0].decode()
                             for i in range(n.value)]
        return out

    def set_comm_overlap(self, on: bool) -> None:
        """The overlapped logits gather (next forward's second batch part runs during it)."""
        check(lib().l3_comm_set_overlap(self._h, int(bool(on))))

    def comm_barrier(self) -> None:
        check(lib().l3_comm_barrier(self._h))

    def comm_max(self, x: float) -> float:
        v = ctypes.c_double(x)
        check(lib().l3_comm_allreduce_max(self._h, ctypes.byref(v)))
        return v.value

    # ---- ops ----
    def op_softmax(self, x: np.ndarray) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.float32)
        y = np.empty_like(x)
        n = x.shape[-1]
        check(lib().l3_op_softmax_host(self._h, ptr(x), x.size // n, n, ptr(y)))
        return y

    def op_argmax(self, x: np.ndarray) -> np.ndarray:
        """argmax over the last axis (np.argmax tie-break, NaN first); int32 of x.shape[:-1]."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        n = x.shape[-1]
        out = np.empty(x.shape[:-1], np.int32)
        check(lib().l3_op_argmax_host(self._h, ptr(x), x.size // n, n, ptr(out)))
        return out

    def op_sample(self, logits: np.ndarray, temperature: float, top_k: int = 0, top_p: float = 1.0,
                  u: Optional[np.ndarray] = None, seed: int = 0, row0: int = 0, pos: int = 0) -> np.ndarray:
        """One sampled id per row of ``logits`` (last axis) by the rule of ``set_sampling``; int32
        of logits.shape[:-1].  ``u``: one uniform in [0, 1) per row; None: row r draws
        ``sample_uniform(seed, row0 + r, pos)`` on the device."""
        x = np.ascontiguousarray(logits, dtype=np.float32)
        n = x.shape[-1]
        rows = x.size // n
        out = np.empty(x.shape[:-1], np.int32)
        if u is not None:
            u = np.ascontiguousarray(u, dtype=np.float32)
            if u.size != rows:
                raise ValueError(f"u has {u.size} entries for {rows} rows")
        check(lib().l3_op_sample_host(self._h, ptr(x), rows, n, float(temperature), int(top_k), float(top_p),
                                      ptr(u) if u is not None else None, int(seed) & (2 ** 64 - 1),
                                      int(row0), int(pos), ptr(out)))
        return out

    def op_silu(self, x: np.ndarray) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.float32)
        y = np.empty_like(x)
        check(lib().l3_op_silu_host(self._h, ptr(x), x.size, ptr(y)))
        return y

    def op_rmsnorm(self, x: np.ndarray, w: np.ndarray, eps: float) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.float32)
        w = np.ascontiguousarray(w, dtype=np.float32)
        y = np.empty_like(x)
        n = x.shape[-1]
        check(lib().l3_op_rmsnorm_host(self._h, ptr(x), ptr(w), x.size // n, n, eps, ptr(y)))
        return y

    def op_rope(self, x: np.ndarray, cos_t: np.ndarray, sin_t: np.ndarray) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.float32)
        c = np.ascontiguousarray(cos_t, dtype=np.float32)
        s = np.ascontiguousarray(sin_t, dtype=np.float32)
        B, L, nh, hd = x.shape
        y = np.empty_like(x)
        check(lib().l3_op_rope_host(self._h, ptr(x), B, L, nh, hd, ptr(c), ptr(s), ptr(y)))
        return y

    def op_linear(self, x: np.ndarray, w: np.ndarray) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.float32)
        w = np.ascontiguousarray(w, dtype=np.float32)
        K = x.shape[-1]
        N = w.shape[0]
        y = np.empty(x.shape[:-1] + (N,), np.float32)
        check(lib().l3_op_linear_host(self._h, ptr(x), x.size // K, K, N, ptr(w), ptr(y)))
        return y

    def op_to_bf16(self, x: np.ndarray):
        """(uint16 array of x's shape, count): the device bf16 conversion of l3_set_weight_bf16
        (round-to-nearest-even, ``utils.round_bf16``'s rule) and how many elements it changed."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        out = np.empty(x.shape, np.uint16)
        n = ctypes.c_int64(0)
        check(lib().l3_op_to_bf16_host(self._h, ptr(x), x.size, ptr(out), ctypes.byref(n)))
        return out, int(n.value)

    def op_linear_bf16(self, x: np.ndarray, w_u16: np.ndarray, norm_w: Optional[np.ndarray] = None,
                       eps: float = 0.0) -> np.ndarray:
        """``x [rows <= 8, K] @ W.T`` with W [N, K] given as bf16 bit patterns (uint16), on the
        bf16-weight GEMV (l3_op_linear_bf16_host); with ``norm_w`` the RMSNorm of x (weight norm_w,
        ``eps``) is applied first.  A shape that kernel does not take raises."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        w = np.ascontiguousarray(w_u16, dtype=np.uint16)
        if x.ndim != 2 or w.ndim != 2 or w.shape[1] != x.shape[1]:
            raise ValueError(f"x {x.shape} and w {w.shape} must be [rows, K] and [N, K]")
        g = None if norm_w is None else np.ascontiguousarray(norm_w, dtype=np.float32)
        if g is not None and g.shape != (x.shape[1],):
            raise ValueError(f"norm_w {g.shape} must be [K = {x.shape[1]}]")
        y = np.empty((x.shape[0], w.shape[0]), np.float32)
        check(lib().l3_op_linear_bf16_host(self._h, ptr(x), x.shape[0], x.shape[1], w.shape[0], ptr(w),
                                           ptr(g) if g is not None else None, float(eps), ptr(y)))
        return y

    def op_linear_bf16_rows(self, x: np.ndarray, w_u16: np.ndarray, norm_w: Optional[np.ndarray] = None,
                            eps: float = 0.0) -> np.ndarray:
        """``x [2 <= rows <= 64, K] @ W.T`` with W [N, K] given as bf16 bit patterns (uint16), on the
        weight-streaming MFMA kernel of ``set_weight_bf16_rows`` (l3_op_linear_bf16_rows_host); with
        ``norm_w`` the RMSNorm of x (weight norm_w, ``eps``) is applied first.  A shape that kernel
        does not take raises."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        w = np.ascontiguousarray(w_u16, dtype=np.uint16)
        if x.ndim != 2 or w.ndim != 2 or w.shape[1] != x.shape[1]:
            raise ValueError(f"x {x.shape} and w {w.shape} must be [rows, K] and [N, K]")
        g = None if norm_w is None else np.ascontiguousarray(norm_w, dtype=np.float32)
        if g is not None and g.shape != (x.shape[1],):
            raise ValueError(f"norm_w {g.shape} must be [K = {x.shape[1]}]")
        y = np.empty((x.shape[0], w.shape[0]), np.float32)
        check(lib().l3_op_linear_bf16_rows_host(self._h, ptr(x), x.shape[0], x.shape[1], w.shape[0], ptr(w),
                                                ptr(g) if g is not None else None, float(eps), ptr(y)))
        return y

    def op_to_fp8_rows(self, x: np.ndarray):
        """(codes uint8 [rows, K], scale float32 [rows], count): the device conversion of
        l3_set_weight_fp8 (``utils.quant_fp8_rows``'s rule) and how many elements differ from
        ``scale * float(code)``."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 2:
            raise ValueError(f"x {x.shape} must be [rows, K]")
        codes = np.empty(x.shape, np.uint8)
        scale = np.empty(x.shape[0], np.float32)
        n = ctypes.c_int64(0)
        check(lib().l3_op_to_fp8_rows_host(self._h, ptr(x), x.shape[0], x.shape[1], ptr(codes), ptr(scale),
                                           ctypes.byref(n)))
        return codes, scale, int(n.value)

    def _op_linear_fp8(self, fn, x, codes, scale, norm_w, eps, route):
        x = np.ascontiguousarray(x, dtype=np.float32)
        w = np.ascontiguousarray(codes, dtype=np.uint8)
        s = np.ascontiguousarray(scale, dtype=np.float32)
        if x.ndim != 2 or w.ndim != 2 or w.shape[1] != x.shape[1]:
            raise ValueError(f"x {x.shape} and codes {w.shape} must be [rows, K] and [N, K]")
        if s.shape != (w.shape[0],):
            raise ValueError(f"scale {s.shape} must be [N = {w.shape[0]}]")
        g = None if norm_w is None else np.ascontiguousarray(norm_w, dtype=np.float32)
        if g is not None and g.shape != (x.shape[1],):
            raise ValueError(f"norm_w {g.shape} must be [K = {x.shape[1]}]")
        y = np.empty((x.shape[0], w.shape[0]), np.float32)
        rt = (ctypes.c_int32 * 6)()
        check(fn(self._h, ptr(x), x.shape[0], x.shape[1], w.shape[0], ptr(w), ptr(s),
                 ptr(g) if g is not None else None, float(eps), ptr(y), rt))
        if not route:
            return y
        fam = GEMM_FAMILIES[rt[0]]
        return y, {"family": fam, **dict(zip(_ROUTE_FIELDS[fam], list(rt)[1:]))}

    def op_linear_fp8(self, x: np.ndarray, codes: np.ndarray, scale: np.ndarray,
                      norm_w: Optional[np.ndarray] = None, eps: float = 0.0, route: bool = False):
        """``x [rows <= 8, K] @ W_q.T`` with ``W_q[n, k] = scale[n] * e4m3fn(codes[n, k])`` (uint8
        codes, power-of-two scales), on the GEMV's fp8 form (l3_op_linear_fp8_host); with ``norm_w``
        the RMSNorm of x (weight norm_w, ``eps``) is applied first.  A shape that kernel does not
        take, a NaN code or a scale that is no power of two raises.  ``route=True``: also the
        launch's route report."""
        return self._op_linear_fp8(lib().l3_op_linear_fp8_host, x, codes, scale, norm_w, eps, route)

    def op_linear_fp8_rows(self, x: np.ndarray, codes: np.ndarray, scale: np.ndarray,
                           norm_w: Optional[np.ndarray] = None, eps: float = 0.0, route: bool = False):
        """The same product for ``2 <= rows <= 64`` on the fp8 form of the weight-streaming MFMA
        kernel of ``set_weight_bf16_rows`` (l3_op_linear_fp8_rows_host), one launch."""
        return self._op_linear_fp8(lib().l3_op_linear_fp8_rows_host, x, codes, scale, norm_w, eps, route)

    def op_linear_logprob(self, x: np.ndarray, w: np.ndarray, targets: np.ndarray):
        """The scoring lm_head on a plain product (l3_op_linear_logprob_host): for the rows of
        ``x @ w.T`` and int targets (-1: none), (logprob float32, lse float32, argmax int32), each
        of shape x.shape[:-1]; the logits are never written."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        w = np.ascontiguousarray(w, dtype=np.float32)
        t = np.ascontiguousarray(targets, dtype=np.int32)
        K = x.shape[-1]
        N = w.shape[0]
        if t.shape != x.shape[:-1]:
            raise ValueError(f"targets {t.shape} for rows {x.shape[:-1]}")
        lp = np.empty(t.shape, np.float32)
        lse = np.empty(t.shape, np.float32)
        am = np.empty(t.shape, np.int32)
        check(lib().l3_op_linear_logprob_host(self._h, ptr(x), x.size // K, K, N, ptr(w), ptr(t), ptr(lp),
                                              ptr(lse), ptr(am)))
        return lp, lse, am

    def op_gemm(self, epi: int, x: np.ndarray, w=None, *, gate_up=None, c=None, norm: bool = False,
                eps: float = 0.0, norm_w=None, a_rows=None, res_src=None, res_rows=None, qkv: Optional[dict] = None,
                ws_floats: int = 0, force_skinny: bool = False, force_tiled: int = 0, x6: bool = False,
                bf16: bool = False, wb_rows: int = 0, wb_min_bytes: int = 0) -> dict:
        """One GEMM launch with epilogue ``epi`` through the library's dispatcher (l3_op_gemm_host).

        ``x`` [M, K] (or the table ``a_rows`` [M] gathers from), ``w`` [N, K]; EPI_SWIGLU takes
        ``gate_up=(wg, wu)`` instead and builds the fused layout.  ``c`` [M, N]: EPI_RESID's
        residual / the initial contents of the output (default: the sentinel).  EPI_QKV takes
        ``qkv`` = dict(L, start_pos, H, KVH, HD, Smax, q_scale, rope_cos, rope_sin, cache_k, cache_v
        [B, KVH, Smax, HD], and optionally col_base, q_out [M, H * HD]).

        Returns a dict: ``route`` (family and the instantiation's parameters), and the outputs WITH
        their guard space — ``c`` [M + 1, ldc], or ``q_out`` [M + 1, H * HD] and ``cache_k`` /
        ``cache_v`` [B + 1, KVH, Smax, HD]; the guard was filled with ``gemm_sentinel(shape, 7)``
        (c, q_out) and ``gemm_sentinel(shape, 8 / 9)`` (cache_k / cache_v).  A launch the
        dispatcher refuses raises."""
        op = GemmOp()
        out, keep = self._fill_gemm_op(op, epi, x, w, gate_up=gate_up, c=c, norm=norm, eps=eps, norm_w=norm_w,
                                       a_rows=a_rows, res_src=res_src, res_rows=res_rows, qkv=qkv, ws_floats=ws_floats,
                                       force_skinny=force_skinny, force_tiled=force_tiled, x6=x6, bf16=bf16,
                                       wb_rows=wb_rows, wb_min_bytes=wb_min_bytes)
        check(lib().l3_op_gemm_host(self._h, ctypes.byref(op)))
        del keep
        out["route"] = _gemm_route(op)
        return out

    @staticmethod
    def _fill_gemm_op(op, epi, x, w, *, gate_up=None, c=None, norm=False, eps=0.0, norm_w=None, a_rows=None,
                      res_src=None, res_rows=None, qkv=None, ws_floats=0, force_skinny=False, force_tiled=0, x6=False,
                      bf16=False, wb_rows=0, wb_min_bytes=0, table=False):
        """The operands of op_gemm into ``op`` (a GemmOp): (out, keep) — the in / out buffers with their
        guard space, and the arrays the struct points into.  ``table``: x is a table [rows, K] and M = 1
        (op_decode_gemm's amax_in selects the row)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        if epi == EPI_SWIGLU and gate_up is not None:
            w = interleave_gate_up(np.asarray(gate_up[0], np.float32), np.asarray(gate_up[1], np.float32))
        w = np.ascontiguousarray(w, dtype=np.float32)
        if x.ndim != 2 or w.ndim != 2 or w.shape[1] != x.shape[1]:
            raise ValueError(f"x {x.shape} and w {w.shape} must be [rows, K] and [N, K]")
        keep = [x, w]
        op.struct_size = ctypes.sizeof(GemmOp)
        op.epi = epi
        N, K = w.shape
        M = 1 if table else x.shape[0]
        if a_rows is not None:
            ar = np.ascontiguousarray(a_rows, dtype=np.int32)
            keep.append(ar)
            M = ar.shape[0]
            op.a_rows = ptr(ar)
        op.M, op.N, op.K = M, N, K
        op.x, op.w, op.x_rows = ptr(x), ptr(w), x.shape[0]
        op.norm, op.eps = int(bool(norm)), float(eps)
        if norm_w is not None:
            g = np.ascontiguousarray(norm_w, dtype=np.float32)
            if g.shape != (K,):
                raise ValueError(f"norm_w {g.shape} must be [K = {K}]")
            keep.append(g)
            op.norm_w = ptr(g)
        out = {}
        if epi != EPI_QKV:
            ldc = N // 2 if epi == EPI_SWIGLU else N
            cbuf = np.empty((M + 1, ldc), np.float32)
            cbuf[:M] = gemm_sentinel((M, ldc), 6) if c is None else np.asarray(c, np.float32).reshape(M, ldc)
            cbuf[M:] = gemm_sentinel((1, ldc), 7)
            out["c"] = cbuf
            op.c, op.c_rows = ptr(cbuf), M + 1
            if res_src is not None:
                rs = np.ascontiguousarray(res_src, dtype=np.float32)
                if rs.ndim != 2 or rs.shape[1] != ldc:
                    raise ValueError(f"res_src {rs.shape} must be [rows, {ldc}]")
                keep.append(rs)
                op.res_src, op.res_src_rows = ptr(rs), rs.shape[0]
            if res_rows is not None:
                rr = np.ascontiguousarray(res_rows, dtype=np.int32)
                if rr.shape != (M,):
                    raise ValueError(f"res_rows {rr.shape} must be [M = {M}]")
                keep.append(rr)
                op.res_rows = ptr(rr)
        else:
            q = dict(qkv)
            L, H, KVH, HD, Smax = (int(q[k]) for k in ("L", "H", "KVH", "HD", "Smax"))
            if L < 1 or M % L:
                raise ValueError(f"M = {M} rows are not whole sequences of L = {L}")
            B = M // L
            cos = np.ascontiguousarray(q["rope_cos"], dtype=np.float32)
            sin = np.ascontiguousarray(q["rope_sin"], dtype=np.float32)
            if cos.shape != (Smax, HD // 2) or sin.shape != cos.shape:
                raise ValueError(f"rope tables {cos.shape} / {sin.shape} must be [Smax, HD / 2]")
            keep += [cos, sin]
            qbuf = np.empty((M + 1, H * HD), np.float32)
            qbuf[:M] = gemm_sentinel((M, H * HD), 5) if q.get("q_out") is None else np.asarray(q["q_out"], np.float32)
            qbuf[M:] = gemm_sentinel((1, H * HD), 7)
            caches = []
            for name, salt in (("cache_k", 8), ("cache_v", 9)):
                buf = np.empty((B + 1, KVH, Smax, HD), np.float32)
                buf[:B] = np.asarray(q[name], np.float32).reshape(B, KVH, Smax, HD)
                buf[B:] = gemm_sentinel((1, KVH, Smax, HD), salt)
                caches.append(buf)
            out.update(q_out=qbuf, cache_k=caches[0], cache_v=caches[1])
            op.L, op.start_pos, op.H, op.KVH, op.HD, op.Smax = L, int(q["start_pos"]), H, KVH, HD, Smax
            op.col_base, op.cache_B, op.q_scale = int(q.get("col_base", 0)), B + 1, float(q["q_scale"])
            op.rope_cos, op.rope_sin = ptr(cos), ptr(sin)
            op.q_out, op.q_rows, op.cache_k, op.cache_v = ptr(qbuf), M + 1, ptr(caches[0]), ptr(caches[1])
        op.ws_floats, op.wb_min_bytes = int(ws_floats), int(wb_min_bytes)
        op.force_skinny, op.force_tiled, op.x6 = int(bool(force_skinny)), int(force_tiled), int(bool(x6))
        op.bf16, op.wb_rows = int(bool(bf16)), int(wb_rows)
        return out, keep

    def op_decode_gemm(self, epi: int, x: np.ndarray, w=None, *, storage: str = "fp32", parts=None, nparts=None,
                       x_out: bool = False, amax_part: bool = False, amax_rows: bool = False, amax_nct=None,
                       amax_in=None, amax_in_n=None, amax_ids: bool = True, state: Optional[DecState] = None,
                       pos_adv: bool = False, kv_bak: bool = False, pos_dev: bool = False, **kw) -> dict:
        """One GEMM launch as ``op_gemm`` (its arguments in ``kw``), with the arguments of a captured
        greedy decode step (l3_op_decode_gemm_host).

        ``storage``: "fp32", "bf16" (the entry rounds ``w``) or "fp8" (``utils.quant_fp8_rows(w)`` goes
        in, and ``w`` itself becomes ``scale * e4m3fn(codes)``); with a norm both take ``norm_w``.
        ``parts`` [M, P, D]: the O-proj partial rows (``nparts``: the count passed, default P); a
        guard row ``gemm_sentinel((1, D), 12)`` follows them.  ``x_out`` / ``amax_part`` /
        ``amax_rows`` / ``kv_bak``: ask for that output.  ``amax_in``: ARGMAX_PART [n] candidates,
        ``x`` then is the table the winner indexes and M = 1 (``amax_in_n``: the count passed;
        ``amax_ids=False``: no id buffer).  ``state``: a DecState, updated in place; ``pos_adv`` /
        ``pos_dev`` use it.

        Returns op_gemm's dict plus, WITH their guard space and starting as sentinels: ``x_out``
        [M + 1, K] (``gemm_sentinel(.., 13)``), ``amax_part`` [N / 4 + 4] and ``amax_blocks``,
        ``amax_rows`` [M + 1, nct] (both ``argmax_parts_sentinel(.., 1 / 2)``), ``amax_ids`` [2]
        (``int_sentinel(2, 5)``), ``kv_bak`` [33, 2, B, KVH, HD] (``gemm_sentinel(.., 14)``), and with
        fp8 storage ``w_model``, the weights the codes stand for."""
        import utils

        if storage not in STORAGES:
            raise ValueError(f"storage {storage!r} is none of {sorted(STORAGES)}")
        d = DecodeGemmOp()
        d.struct_size = ctypes.sizeof(DecodeGemmOp)
        d.storage = STORAGES[storage]
        extra = {}
        hold = []
        if epi == EPI_SWIGLU and kw.get("gate_up") is not None:
            gu = kw.pop("gate_up")
            w = interleave_gate_up(np.asarray(gu[0], np.float32), np.asarray(gu[1], np.float32))
        if storage == "fp8":
            codes, scale = utils.quant_fp8_rows(w)
            w = (utils.fp8_e4m3_table()[codes] * scale[:, None]).astype(np.float32)
            hold += [codes, scale]
            d.wq_codes, d.wq_scale = ptr(codes), ptr(scale)
            extra["w_model"] = w
        out, keep = self._fill_gemm_op(d.g, epi, x, w, table=amax_in is not None, **kw)
        M, N, K = d.g.M, d.g.N, d.g.K
        if parts is not None:
            p = np.asarray(parts, np.float32)
            D = N if epi == EPI_RESID else K
            if p.ndim != 3 or p.shape[0] != M or p.shape[2] != D:
                raise ValueError(f"parts {p.shape} must be [M = {M}, P, D = {D}]")
            pbuf = np.concatenate([p.reshape(-1, D), gemm_sentinel((1, D), 12)])
            hold.append(pbuf)
            d.parts, d.parts_rows = ptr(pbuf), pbuf.shape[0]
            d.nparts = p.shape[1] if nparts is None else int(nparts)
        if x_out:
            xo = gemm_sentinel((M + 1, K), 13).copy()
            extra["x_out"] = xo
            d.x_out, d.x_out_rows = ptr(xo), M + 1
        if amax_part:
            ap = argmax_parts_sentinel(N // 4 + 4, 1)
            extra["amax_part"] = ap
            d.amax_part, d.amax_part_n = ptr(ap), ap.shape[0]
        if amax_rows:
            nct = (N + 63) // 64 if amax_nct is None else int(amax_nct)
            ar = argmax_parts_sentinel((M + 1, max(nct, 1)), 2)
            extra["amax_rows"] = ar
            d.amax_rows, d.amax_rows_rows, d.amax_nct = ptr(ar), M + 1, nct
        if amax_in is not None:
            ai = np.ascontiguousarray(amax_in, dtype=ARGMAX_PART)
            hold.append(ai)
            d.amax_in = ptr(ai)
            d.amax_in_n = ai.shape[0] if amax_in_n is None else int(amax_in_n)
            if amax_ids:
                ids = int_sentinel(2, 5)
                extra["amax_ids"] = ids
                d.amax_ids = ptr(ids)
        io = None
        if state is not None:
            io = state._io()
            d.state = ctypes.pointer(io)
        d.pos_adv, d.pos_dev = int(bool(pos_adv)), int(bool(pos_dev))
        if kv_bak:
            B = M // d.g.L
            kb = gemm_sentinel((KV_BAK_SLOTS + 1, 2, B, d.g.KVH, d.g.HD), 14).copy()
            extra["kv_bak"] = kb
            d.kv_bak = ptr(kb)
        check(lib().l3_op_decode_gemm_host(self._h, ctypes.byref(d)))
        del keep, hold
        if state is not None:
            state._take(io)
        out.update(extra)
        out["route"] = _gemm_route(d.g)
        if amax_part:
            out["amax_blocks"] = int(d.amax_blocks)
        return out

    def op_argmax_parts(self, parts: np.ndarray, hist_off: int = 0, state: Optional[DecState] = None) -> np.ndarray:
        """The decode loop's argmax over per-block candidates (l3_op_argmax_parts_host): ``parts``
        ARGMAX_PART [rows, n] -> ids int32 [rows + 1] WITH a guard entry (``int_sentinel(rows + 1, 6)``
        before the launch).  ``state`` (a DecState of that many rows) is updated in place."""
        p = np.ascontiguousarray(parts, dtype=ARGMAX_PART)
        if p.ndim != 2:
            raise ValueError(f"parts {p.shape} must be [rows, n]")
        if state is not None and state.rows != p.shape[0]:
            raise ValueError(f"a state of {state.rows} rows for {p.shape[0]} rows of candidates")
        ids = int_sentinel(p.shape[0] + 1, 6)
        io = state._io() if state is not None else None
        check(lib().l3_op_argmax_parts_host(self._h, ptr(p), p.shape[0], p.shape[1], int(hist_off),
                                            ctypes.byref(io) if io is not None else None, ptr(ids)))
        if state is not None:
            state._take(io)
        return ids

    def op_kv_restore(self, cache: np.ndarray, bak: np.ndarray, pos: int) -> np.ndarray:
        """The unguarded undo of one cache's append (l3_op_kv_restore_host): ``cache`` [B + 1, KVH,
        Smax, HD] WITH its guard sequence, ``bak`` [B, KVH, HD]; returns the cache after the launch."""
        ck = np.array(cache, dtype=np.float32, order="C")
        b = np.ascontiguousarray(bak, dtype=np.float32)
        if ck.ndim != 4 or b.shape != (ck.shape[0] - 1, ck.shape[1], ck.shape[3]):
            raise ValueError(f"cache {ck.shape} must be [B + 1, KVH, Smax, HD] and bak {b.shape} [B, KVH, HD]")
        check(lib().l3_op_kv_restore_host(self._h, ptr(ck), ck.shape[0], ptr(b), b.shape[0], ck.shape[1], ck.shape[2],
                                          ck.shape[3], int(pos)))
        return ck

    def op_decode_persist(self, token: int, state: DecState, *, steps: int = 1, kv_bak: bool = False) -> dict:
        """One persistent decode step (``steps`` 2: two chained launches) launched directly, with every
        stage's output (l3_op_decode_persist_host).  ``state``: a one-row DecState at the step's
        position, updated in place.  Returns ``tags`` / ``vals`` per layer as dicts of the stages
        ``qkv, o, h1, hid, h2`` (uint32 / float32 arrays, the LAST launch's granules), ``lm_tag`` [256, 2],
        ``lm_val`` float32 [256] and ``lm_idx`` int32 [256] (the lm partial granules), ``epoch`` [3],
        ``tag``, ``err``, ``id``, ``kv_bak`` [n_layers, 8, 32, 2, KVH, HD] (``gemm_sentinel(.., 14)``
        before the launch; a layer's block [0] holds the one-sequence slots [32][k, v][KVH][HD], the
        other seven are the room of the batched layout and stay untouched) or None, and ``route``: ``instance`` (NCD, NCF, KPF, LMPF), ``grid``, ``GL``."""
        d = self.dims
        H, KVH, D, FD, nl = d.n_heads, d.n_kv_heads, d.dim, d.hidden_dim, d.n_layers
        HD = D // H
        sizes = [("qkv", (H + 2 * KVH) * HD), ("o", H * HD), ("h1", D), ("hid", FD), ("h2", D)]
        slab = sum(n for _, n in sizes)
        if state.rows != 1:
            raise ValueError("a one-row state")
        op = DecodePersistOp()
        op.struct_size = ctypes.sizeof(DecodePersistOp)
        op.token, op.steps, op.use_kv_bak = int(token), int(steps), int(bool(kv_bak))
        gran = np.zeros(nl * slab, np.uint64)
        lm = np.zeros(512, np.uint64)
        op.gran, op.gran_n, op.lm_parts = ptr(gran), gran.size, ptr(lm)
        kb = None
        if kv_bak:
            kb = gemm_sentinel((nl, 8, KV_BAK_SLOTS, 2, KVH, HD), 14).copy()
            op.kv_bak, op.kv_bak_n = ptr(kb), kb.size
        io = state._io()
        op.state = ctypes.pointer(io)
        check(lib().l3_op_decode_persist_host(self._h, ctypes.byref(op)))
        state._take(io)
        g = gran.reshape(nl, slab)
        tags, vals = [], []
        for l in range(nl):
            o, t, v = 0, {}, {}
            for name, n in sizes:
                t[name] = (g[l, o:o + n] >> np.uint64(32)).astype(np.uint32)
                v[name] = (g[l, o:o + n] & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.float32)
                o += n
            tags.append(t)
            vals.append(v)
        lo = (lm & np.uint64(0xFFFFFFFF)).astype(np.uint32).reshape(256, 2)
        return {
            "tags": tags, "vals": vals, "lm_tag": (lm >> np.uint64(32)).astype(np.uint32).reshape(256, 2),
            "lm_val": lo[:, 0].copy().view(np.float32), "lm_idx": lo[:, 1].copy().view(np.int32),
            "epoch": [int(x) for x in op.epoch], "tag": int(op.tag), "err": int(op.err), "id": int(op.id_out),
            "kv_bak": kb,
            "route": {"instance": tuple(int(x) for x in op.route[:4]), "grid": int(op.route[4]), "GL": int(op.route[5])},
        }

    def op_attention(self, q, cache_k, cache_v, start_pos: int, n_heads: int, *, last: bool = False,
                     pos_dev: bool = False, wo=None, out=None, scaled: bool = False):
        """One dense attention launch through the library's dispatcher (l3_op_attention_host).

        ``q`` [B, L, H * HD]: the plain queries, multiplied here in fp32 by log2(e) / sqrt(HD)
        (``attn_scale_q``), or with ``scaled`` what the kernel takes as it is.  ``cache_k`` /
        ``cache_v`` [B, KVH, Smax, HD].  ``last``: the last-rows launch of a pruned last block;
        ``pos_dev``: the position is read from a device word; ``wo`` [D, H * HD]: the decode launch
        with the O-proj fused.  ``out`` [B * L, H * HD] (with ``wo``: [B, H * D]): the initial
        contents of the output (default: ``gemm_sentinel(shape, 6)``); a float32 array of the
        returned shape is used in place, guard row and all.

        Returns (out, route): ``out`` [B * L + 1, width] WITH its guard row, which was filled with
        ``gemm_sentinel((1, width), 7)``; ``route`` a dict — kernel ("prefill", "decode",
        "decode_oproj"), hd, qbw, g, kt (0 for the decode kernels) and grid (x, y, z).  A launch
        the dispatcher refuses raises and leaves ``out`` as it was."""
        ck = np.ascontiguousarray(cache_k, dtype=np.float32)
        cv = np.ascontiguousarray(cache_v, dtype=np.float32)
        if ck.ndim != 4 or cv.shape != ck.shape:
            raise ValueError(f"cache_k {ck.shape} / cache_v {cv.shape} must be [B, KVH, Smax, HD]")
        B, KVH, Smax, HD = ck.shape
        H = int(n_heads)
        q = np.asarray(q, dtype=np.float32)
        if q.ndim != 3 or q.shape[0] != B or q.shape[2] != H * HD:
            raise ValueError(f"q {q.shape} must be [B = {B}, L, H * HD = {H * HD}]")
        L = q.shape[1]
        q = np.ascontiguousarray(q if scaled else attn_scale_q(q, HD))
        D = 0
        w = None
        if wo is not None:
            w = np.ascontiguousarray(wo, dtype=np.float32)
            if w.ndim != 2 or w.shape[1] != H * HD:
                raise ValueError(f"wo {w.shape} must be [D, H * HD = {H * HD}]")
            D = w.shape[0]
        width = H * D if w is not None else H * HD
        if isinstance(out, np.ndarray) and out.shape == (B * L + 1, width) and out.dtype == np.float32 \
                and out.flags.c_contiguous:
            buf = out  # the caller's own buffer, guard row included, used in place
        else:
            buf = np.empty((B * L + 1, width), np.float32)
            buf[:B * L] = gemm_sentinel((B * L, width), 6) if out is None \
                else np.asarray(out, np.float32).reshape(B * L, width)
            buf[B * L:] = gemm_sentinel((1, width), 7)
        r = np.zeros(8, np.int32)
        check(lib().l3_op_attention_host(self._h, ptr(q), ptr(ck), ptr(cv), B, L, int(start_pos), H, KVH, HD, Smax,
                                         int(bool(last)) | (int(bool(pos_dev)) << 1), None if w is None else ptr(w), D,
                                         ptr(buf), B * L + 1, ptr(r)))
        route = {"kernel": ATTN_KERNELS[int(r[0])], "hd": int(r[1]), "qbw": int(r[2]), "g": int(r[3]), "kt": int(r[4]),
                 "grid": (int(r[5]), int(r[6]), int(r[7]))}
        return buf, route

    def op_ffn_block(self, x: np.ndarray, wg: np.ndarray, wu: np.ndarray, wd: np.ndarray, norm: bool,
                     fused: bool) -> np.ndarray:
        """Extension (l3_op_ffn_block_host): x + down(SwiGLU(f(x) * x @ Wgu.T)) over more than 256
        rows, f the RMSNorm row factor (norm) or 1, on the fused kernel (an error where it does
        not take the shape) or on the two tiled fp32 launches."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        D = x.shape[-1]
        FD = wg.shape[0]
        y = np.empty_like(x)
        wg, wu, wd = (np.ascontiguousarray(a, dtype=np.float32) for a in (wg, wu, wd))
        check(lib().l3_op_ffn_block_host(self._h, ptr(x), x.size // D, D, FD, ptr(wg), ptr(wu), ptr(wd),
                                         int(bool(norm)), int(bool(fused)), ptr(y)))
        return y

    def op_ffn(self, x: np.ndarray, wg: np.ndarray, wu: np.ndarray, wd: np.ndarray) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.float32)
        D = x.shape[-1]
        FD = wg.shape[0]
        y = np.empty_like(x)
        wg, wu, wd = (np.ascontiguousarray(a, dtype=np.float32) for a in (wg, wu, wd))
        check(lib().l3_op_ffn_host(self._h, ptr(x), x.size // D, D, FD, ptr(wg), ptr(wu), ptr(wd),
                                   ptr(y)))
        return y


def member_rows(B: int, n: int, i: int) -> int:
    """Rows of group member i (of n) in a batch of B: global rows i, i + n, i + 2n, ... — the
    l3_group row mapping (row r on member r % n as its local row r // n), which does not depend
    on B, so a row's KV cache stays on one device across calls of any batch size."""
    if n <= 0 or not 0 <= i < n:
        raise ValueError(f"bad member {i} of {n}")
    return (B - i + n - 1) // n if B > i else 0


class Group:
    """One process driving ``devices`` (l3_group_*, include/llama3hip.h): one context per
    device, RCCL communicators from ncclCommInitAll, batch row r on member r % n (its local
    row r // n).  Same upload / finalize / forward / greedy_step surface as ``Context``."""

    def __init__(self, dims: Dims, devices):
        devs = np.ascontiguousarray(list(devices), dtype=np.int32)
        if devs.ndim != 1 or devs.size == 0:
            raise ValueError("devices must be a non-empty list of device ordinals")
        self._h = ctypes.c_void_p()
        check(lib().l3_group_create(int(devs.size), ptr(devs), ctypes.byref(dims), ctypes.byref(self._h)))
        self.dims = dims
        self.devices = [int(x) for x in devs]
        self.n = len(self.devices)
        local = Dims.from_buffer_copy(dims)
        local.max_batch_size = -(-dims.max_batch_size // self.n)
        self.members = []
        for i, dv in enumerate(self.devices):
            h = ctypes.c_void_p()
            check(lib().l3_group_context(self._h, i, ctypes.byref(h)))
            m = Context._member(h, local, dv, self)
            m.nranks, m.rank = self.n, i  # its communicator (ncclCommInitAll), used via the group
            self.members.append(m)

    def close(self):
        if self._h:
            for m in self.members:
                m._h = ctypes.c_void_p()
            lib().l3_group_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def rows(self, B: int, i: int) -> int:
        """Rows of member i in a batch of B (rows i, i + n, ...)."""
        return member_rows(B, self.n, i)

    def upload(self, layer: int, kind: int, w: np.ndarray) -> None:
        a = np.ascontiguousarray(w, dtype=np.float32)
        rows, cols = (1, a.shape[0]) if a.ndim == 1 else a.shape
        check(lib().l3_group_upload_weight(self._h, layer, kind, ptr(a), rows, cols))

    def finalize(self) -> None:
        check(lib().l3_group_finalize(self._h))

    def forward(self, ids: np.ndarray, start_pos: int) -> np.ndarray:
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        B, L = ids.shape
        out = pinned.empty((B, self.dims.vocab_size), np.float32)
        check(lib().l3_group_forward_host(self._h, ptr(ids), B, L, start_pos, ptr(out)))
        return out

    def forward_dev(self, ids_dev, B: int, L: int, start_pos: int, logits_dev: int) -> None:
        """ids_dev: one device pointer per member (its rows, int32); logits_dev on member 0."""
        arr = (ctypes.c_void_p * self.n)(*[ctypes.c_void_p(p or 0) for p in ids_dev])
        check(lib().l3_group_forward_dev(self._h, arr, B, L, start_pos, logits_dev))

    def greedy_step(self, ids: np.ndarray, start_pos: int, want_logits: bool = False):
        if want_logits:
            raise NotImplementedError("Group.greedy_step returns ids only")
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        B, L = ids.shape
        nxt = np.empty(B, np.int64)
        check(lib().l3_group_greedy_step_host(self._h, ptr(ids), B, L, start_pos, ptr(nxt)))
        return nxt, None

    def set_decode_horizon(self, end_pos: int) -> None:
        self.members[0].set_decode_horizon(end_pos)

    def synchronize(self) -> None:
        check(lib().l3_group_synchronize(self._h))

    def _single(self) -> Context:
        if self.n != 1:
            raise RuntimeError("a per-block call on a multi-device Llama: its KV cache rows are spread "
                               "over the devices; build a TransformerBlock from the weights instead")
        return self.members[0]

    def layer_forward(self, layer: int, x: np.ndarray, start_pos: int) -> np.ndarray:
        return self._single().layer_forward(layer, x, start_pos)

    def attention_forward(self, layer: int, x: np.ndarray, start_pos: int) -> np.ndarray:
        return self._single().attention_forward(layer, x, start_pos)


def launch_key() -> str:
    """Key of the RCCL-id hand-off file: equal on every rank of one launch, different for every
    launch — torchrun's run id (TORCHELASTIC_RUN_ID; "none" under the default static rendezvous,
    so not unique alone), the launcher's pid (torchrun's agent is the parent of every rank it
    starts) and MASTER_PORT.  A launcher that sets L3_LAUNCH_KEY (bench.py's spawn_ranks) names
    the launch itself."""
    own = os.environ.get("L3_LAUNCH_KEY")
    if own:
        return own
    run = os.environ.get("TORCHELASTIC_RUN_ID") or "local"
    return f"{run}_{os.getppid()}_{os.environ.get('MASTER_PORT', '0')}"


def remove_unique_id(key: str) -> None:
    """Rank 0, once every rank has joined the communicator (ncclCommInitRank is collective, so
    every rank has read the id by then): drop the hand-off file."""
    try:
        os.remove(os.path.join("/tmp", f"l3_rccl_uid_{key}"))
    except OSError:
        pass


def exchange_unique_id(rank: int, world: int, key: str, timeout_s: float = 120.0) -> bytes:
    """Ship the 128-byte RCCL id from rank 0 to the other ranks of ONE node through an
    atomically renamed file in /tmp (no PyTorch / gloo needed).  ``key`` must be unique per
    launch and equal on all ranks (e.g. launcher pid + MASTER_PORT)."""
    import time

    path = os.path.join("/tmp", f"l3_rccl_uid_{key}")
    if rank == 0:
        uid = comm_unique_id()
        tmp = f"{path}.{os.getpid()}.tmp"
        with open(tmp, "wb") as f:
            f.write(uid)
        os.replace(tmp, path)
        return uid
    t0 = time.time()
    while True:
        try:
            with open(path, "rb") as f:
                uid = f.read()
            if len(uid) == 128:
                return uid
        except FileNotFoundError:
            pass
        if time.time() - t0 > timeout_s:
            raise RuntimeError(f"timed out waiting for the RCCL id at {path}")
        time.sleep(0.01)


def comm_unique_id() -> bytes:
    buf = (ctypes.c_uint8 * 128)()
    check(lib().l3_comm_unique_id(buf))
    return bytes(buf)


_op_ctx = {}


def op_context(device: int = 0) -> Context:
    """Shared op-only context (n_layers = 0) used by the module-level ops."""
    if device not in _op_ctx:
        d = Dims(dim=64, n_layers=0, n_heads=1, n_kv_heads=1, vocab_size=1, hidden_dim=32,
                 max_seq_len=1, max_batch_size=1, norm_eps=1e-6)
        _op_ctx[device] = Context(d, device)
    return _op_ctx[device]
